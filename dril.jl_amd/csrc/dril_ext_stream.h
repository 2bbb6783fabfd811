// dril_ext_stream.h — what the device-array verbs of a DRIL_ENV_EXTERNAL handle share between the PPO handle (dril_ext.hip: dril_ext_*_device) and the SAC handle
// (dril_sac_ext.hip: dril_sac_ext_*_device): the rule a caller's device pointer must meet, and the hand-over between the caller's stream and the handle's stream.
// Host code only; each handle wraps these with its own error reporting.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

namespace dril {

// an argument of a device verb must be memory the handle's device can address, long enough for the array: a host pointer handed to a kernel is a GPU fault.
// Empty string: fine; otherwise the message of DRIL_ERR_INVALID_ARG
inline std::string ext_ptr_problem(int device, const char* verb, const char* name, const void* p, size_t bytes) {
    hipPointerAttribute_t at{};
    const hipError_t e = hipPointerGetAttributes(&at, p);
    if (e != hipSuccess) (void)hipGetLastError();
    const bool ok = e == hipSuccess && ((at.type == hipMemoryTypeDevice && at.device == device) || at.type == hipMemoryTypeManaged || (at.type == hipMemoryTypeHost && at.devicePointer != nullptr));
    if (!ok) return std::string(verb) + ": " + name + " is not memory of device " + std::to_string(device) + " (the *_device verbs take device arrays; host arrays go to the verbs without the suffix)";
    if (at.type == hipMemoryTypeDevice) {
        hipDeviceptr_t base = nullptr; size_t size = 0;
        if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) != hipSuccess) (void)hipGetLastError();
        else if ((const char*)p + bytes > (const char*)base + size) return std::string(verb) + ": the allocation behind " + name + " ends before the " + std::to_string(bytes) + " bytes of the array";
    }
    return std::string();
}
// the handle's stream takes over from the caller's stream / hands back to it: two events per handle, no host wait
inline hipError_t ext_stream_take(hipStream_t own, hipEvent_t ev_in, void* caller_stream) {
    const hipError_t e = hipEventRecord(ev_in, (hipStream_t)caller_stream);
    return e != hipSuccess ? e : hipStreamWaitEvent(own, ev_in, 0);
}
inline hipError_t ext_stream_give(hipStream_t own, hipEvent_t ev_out, void* caller_stream) {
    const hipError_t e = hipEventRecord(ev_out, own);
    return e != hipSuccess ? e : hipStreamWaitEvent((hipStream_t)caller_stream, ev_out, 0);
}

}  // namespace dril
