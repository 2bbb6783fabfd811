// dril_policy_internal.h — how the training handles (dril_api.hip, dril_sac.hip) hand a device-side snapshot to the deployment policy object (dril_policy.hip)
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/dril_policy.h"

namespace dril {

// every pointer is DEVICE memory of desc.device, read on `stream` (the handle's: the copies are ordered behind whatever the handle has enqueued); the call
// returns once they have completed.  log_std: A floats or null (Categorical); obs_mean / obs_var: D floats each or null (desc.has_norm == 0)
struct PolicyDeviceSource {
    dril_policy_desc desc;
    const float* actor; size_t n;
    const float* log_std; const float* obs_mean; const float* obs_var;
    hipStream_t stream;
};
// status of enum dril_status; on failure *msg holds the reason and nothing is left allocated
int policy_from_device(const PolicyDeviceSource& src, dril_policy** out, std::string* msg);
// the construction error dril_policy_last_error(NULL) reports (set by the from-handle verbs, which live beside their handles)
void policy_set_create_error(const std::string& msg);

}  // namespace dril
