// dril_comm.hip — the PPO handle's communicator: RCCL, dlopen'ed lazily so single-GPU users never load it, the debug loopback group, and the all-reduce that rides the
// handle's stream (dril_comm_*, dril_debug_comm_loopback; include/dril_hip.h)
#include <dlfcn.h>

#include <chrono>
#include <condition_variable>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "dril_handle.h"

using namespace dril;
using namespace dril::ppo;

namespace {
// ---- minimal RCCL surface, resolved at run time ------------------------------------------------
struct RcclApi {
    void* lib = nullptr;
    int (*GetUniqueId)(void*) = nullptr;
    int (*CommInitRank)(void**, int, const void*, int) = nullptr;   // ncclUniqueId passed by value = 128-byte struct
    int (*AllReduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    int (*CommCount)(void*, int*) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
    const char* (*GetLastError)(void*) = nullptr;       // ncclGetLastError(comm): the human-readable cause behind a status code (which rank / device / transport)
};
struct NcclId { char bytes[128]; };
typedef int (*nccl_init_rank_fn)(void**, int, NcclId, int);
RcclApi g_rccl;
bool load_rccl(std::string& err) {
    if (g_rccl.lib) return true;
    const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    for (const char* n : names) { g_rccl.lib = dlopen(n, RTLD_NOW | RTLD_GLOBAL); if (g_rccl.lib) break; }
    if (!g_rccl.lib) { err = std::string("dlopen(librccl) failed: ") + dlerror(); return false; }
    g_rccl.GetUniqueId = (int (*)(void*))dlsym(g_rccl.lib, "ncclGetUniqueId");
    g_rccl.CommInitRank = (int (*)(void**, int, const void*, int))dlsym(g_rccl.lib, "ncclCommInitRank");
    g_rccl.AllReduce = (int (*)(const void*, void*, size_t, int, int, void*, hipStream_t))dlsym(g_rccl.lib, "ncclAllReduce");
    g_rccl.CommDestroy = (int (*)(void*))dlsym(g_rccl.lib, "ncclCommDestroy");
    g_rccl.GetErrorString = (const char* (*)(int))dlsym(g_rccl.lib, "ncclGetErrorString");
    g_rccl.CommCount = (int (*)(void*, int*))dlsym(g_rccl.lib, "ncclCommCount");
    g_rccl.GetLastError = (const char* (*)(void*))dlsym(g_rccl.lib, "ncclGetLastError");
    if (!g_rccl.GetUniqueId || !g_rccl.CommInitRank || !g_rccl.AllReduce) { err = "librccl lacks ncclGetUniqueId/ncclCommInitRank/ncclAllReduce"; return false; }
    return true;
}
constexpr int kNcclSum = 0;
// "<call>: <ncclGetErrorString(rc)> [<ncclGetLastError(comm)>]": a failing first contact with a multi-GPU node must name its cause in dril_last_error
std::string rccl_error(const char* call, int rc, void* comm) {
    std::string m = std::string(call) + ": " + (g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : "error") + " (status " + std::to_string(rc) + ")";
    if (g_rccl.GetLastError) { const char* le = g_rccl.GetLastError(comm); if (le && *le) m += std::string(" [ncclGetLastError: ") + le + "]"; }
    return m;
}

// ---- debug loopback communicator -----------------------------------------------------------------
// RCCL refuses two ranks on one device, so the data-parallel code of the handle (every `reduce` branch of dril_update.hip, dril_api.hip and dril_wrap.hip) could only be
// executed on a multi-GPU node.  A loopback group joins n handles of ONE process on ONE device as ranks 0..n-1: the all-reduce
// call sites, counts and dtypes are unchanged, only the transport differs — the ranks' host threads rendezvous, the last arriver
// makes its stream wait for every rank's buffer, one kernel sums the n device buffers element-wise in rank order and writes the
// sum back to all of them (every rank ends with bit-identical values, as after a ring all-reduce), and the other ranks' streams
// wait for that kernel.  Each handle must be driven from its own host thread (dril_debug_comm_loopback, include/dril_hip.h).
constexpr int kLoopMax = 8;
struct LoopPtrs { void* p[kLoopMax]; };
}  // namespace
namespace dril::ppo {
struct LoopGroup {
    std::mutex mu; std::condition_variable cv;
    int n = 0, arrived = 0, refs = 0; uint64_t gen = 0; int64_t calls = 0;
    LoopPtrs bufs{}; hipEvent_t ready[kLoopMax] = {nullptr}; hipEvent_t done = nullptr;
    size_t count = 0; int dtype = 0; bool mismatch = false, failed = false;
};
}  // namespace dril::ppo
namespace {
template <typename T> __global__ void loop_allreduce_kernel(LoopPtrs bufs, int n, size_t count) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    T s = ((const T*)bufs.p[0])[i];
    for (int r = 1; r < n; ++r) s += ((const T*)bufs.p[r])[i];      // fixed rank order: deterministic
    for (int r = 0; r < n; ++r) ((T*)bufs.p[r])[i] = s;             // this thread has read element i of every rank before it writes any
}

// the loopback transport of one all-reduce (see LoopGroup): called by every rank's host thread with the same count / dtype
int loop_allreduce(dril_handle* h, void* buf, size_t count, int dtype) {
    LoopGroup* g = h->loop; const int r = h->cfg.rank;
    HIPCHK(h, hipEventRecord(g->ready[r], h->stream));                 // this rank's contribution is complete behind this event
    std::unique_lock<std::mutex> lk(g->mu);
    if (g->failed) return fail(h, DRIL_ERR_RCCL, "loopback communicator: an earlier all-reduce failed");
    const uint64_t my_gen = g->gen;
    if (g->arrived == 0) { g->count = count; g->dtype = dtype; g->mismatch = false; }
    else if (g->count != count || g->dtype != dtype) g->mismatch = true;
    g->bufs.p[r] = buf;
    if (++g->arrived == g->n) {
        hipError_t e = hipSuccess;
        for (int q = 0; q < g->n && e == hipSuccess; ++q) e = hipStreamWaitEvent(h->stream, g->ready[q], 0);
        if (e == hipSuccess && !g->mismatch) {
            const unsigned nb = (unsigned)((count + 255) / 256);
            if (dtype == kNcclFloat64) loop_allreduce_kernel<double><<<nb, 256, 0, h->stream>>>(g->bufs, g->n, count);
            else loop_allreduce_kernel<float><<<nb, 256, 0, h->stream>>>(g->bufs, g->n, count);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipEventRecord(g->done, h->stream);
        if (e != hipSuccess || g->mismatch) g->failed = true;
        g->arrived = 0; g->gen += 1; g->calls += 1;
        g->cv.notify_all();
        if (e != hipSuccess) return fail(h, DRIL_ERR_HIP, std::string("loopback all-reduce: ") + hipGetErrorString(e));
    } else {
        if (!g->cv.wait_for(lk, std::chrono::seconds(120), [&] { return g->gen != my_gen; })) {
            g->failed = true; g->arrived = 0; g->gen += 1; g->cv.notify_all();
            return fail(h, DRIL_ERR_RCCL, "loopback all-reduce: the other ranks did not arrive within 120 s (every handle of the group needs its own host thread making the same calls)");
        }
        if (!g->failed) HIPCHK(h, hipStreamWaitEvent(h->stream, g->done, 0));
    }
    if (g->failed) return fail(h, DRIL_ERR_RCCL, g->mismatch ? "loopback all-reduce: the ranks disagree on count / dtype (they are not making the same calls)" : "loopback all-reduce failed on another rank");
    return DRIL_OK;
}
}  // namespace

namespace dril::ppo {
int rccl_allreduce(dril_handle* h, void* buf, size_t count, int dtype) {
    if (!comm_ready(h)) return DRIL_OK;
    h->allreduce_calls += 1;
    prof_begin(h, DRIL_K_ALLREDUCE);
    int rc = 0;
    if (h->loop) { const int lrc = loop_allreduce(h, buf, count, dtype); prof_end(h); return lrc; }
    rc = g_rccl.AllReduce(buf, buf, count, dtype, kNcclSum, h->comm, h->stream);
    prof_end(h);
    if (rc != 0) return fail(h, DRIL_ERR_RCCL, rccl_error("ncclAllReduce", rc, h->comm) + "; " + h->device_info);
    return DRIL_OK;
}
void comm_release(dril_handle* h) {
    if (h->comm && g_rccl.CommDestroy) g_rccl.CommDestroy(h->comm);
    if (h->loop) {                                                   // the last handle to leave frees the group
        LoopGroup* g = h->loop; bool last;
        { std::lock_guard<std::mutex> lk(g->mu); last = --g->refs == 0; }
        if (last) { for (int q = 0; q < g->n; ++q) if (g->ready[q]) hipEventDestroy(g->ready[q]); if (g->done) hipEventDestroy(g->done); delete g; }
        h->loop = nullptr;
    }
}
}  // namespace dril::ppo

// ---- multi-GPU ------------------------------------------------------------------------------------------
DRIL_EXPORT int32_t dril_comm_unique_id(uint8_t id[128]) {
    std::string err;
    if (!id) return fail(nullptr, DRIL_ERR_INVALID_ARG, "null id");
    if (!load_rccl(err)) return fail(nullptr, DRIL_ERR_RCCL, err);
    NcclId nid; std::memset(&nid, 0, sizeof(nid));
    const int rc = g_rccl.GetUniqueId(&nid);
    if (rc != 0) return fail(nullptr, DRIL_ERR_RCCL, rccl_error("ncclGetUniqueId", rc, nullptr));
    std::memcpy(id, nid.bytes, 128);
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_comm_init(dril_handle* h, const uint8_t id[128]) {
    NEED(h); std::string err;
    if (!id) return fail(h, DRIL_ERR_INVALID_ARG, "null id");
    if (!load_rccl(err)) return fail(h, DRIL_ERR_RCCL, err);
    NcclId nid; std::memcpy(nid.bytes, id, 128);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const int rc = ((nccl_init_rank_fn)(void*)g_rccl.CommInitRank)(&h->comm, h->cfg.world_size, nid, h->cfg.rank);
    if (rc != 0) { const std::string m = rccl_error("ncclCommInitRank", rc, nullptr) + "; rank " + std::to_string(h->cfg.rank) + " of " + std::to_string(h->cfg.world_size) + " on " + h->device_info; h->comm = nullptr; return fail(h, DRIL_ERR_RCCL, m); }
    return DRIL_OK;
}

DRIL_EXPORT int32_t dril_debug_comm_loopback(dril_handle** hs, int32_t n) {
    if (!hs || n < 1 || n > kLoopMax) return fail(nullptr, DRIL_ERR_INVALID_ARG, "dril_debug_comm_loopback: 1..8 handles");
    std::vector<bool> seen((size_t)n, false);
    for (int i = 0; i < n; ++i) {
        dril_handle* h = hs[i];
        if (!h) return fail(nullptr, DRIL_ERR_INVALID_ARG, "dril_debug_comm_loopback: null handle");
        if (comm_ready(h)) return fail(h, DRIL_ERR_INVALID_ARG, "dril_debug_comm_loopback: the handle already has a communicator");
        if (h->cfg.world_size != n || h->cfg.rank < 0 || h->cfg.rank >= n || seen[h->cfg.rank]) return fail(h, DRIL_ERR_INVALID_ARG, "dril_debug_comm_loopback: the handles must be ranks 0..n-1 of world_size n, one each");
        if (h->cfg.device != hs[0]->cfg.device) return fail(h, DRIL_ERR_INVALID_ARG, "dril_debug_comm_loopback: all handles must live on one device");
        seen[h->cfg.rank] = true;
    }
    (void)hipSetDevice(hs[0]->cfg.device);
    LoopGroup* g = new LoopGroup(); g->n = n; g->refs = n;
    hipError_t e = hipEventCreateWithFlags(&g->done, hipEventDisableTiming);
    for (int q = 0; q < n && e == hipSuccess; ++q) e = hipEventCreateWithFlags(&g->ready[q], hipEventDisableTiming);
    if (e != hipSuccess) { for (int q = 0; q < n; ++q) if (g->ready[q]) hipEventDestroy(g->ready[q]); if (g->done) hipEventDestroy(g->done); delete g; return fail(hs[0], DRIL_ERR_HIP, hipGetErrorString(e)); }
    for (int i = 0; i < n; ++i) hs[i]->loop = g;
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_comm_ranks(dril_handle* h) {
    if (!h) return -1;
    if (h->loop) return h->loop->n;
    if (h->comm) { int c = -1; if (g_rccl.CommCount && g_rccl.CommCount(h->comm, &c) == 0) return c; return -1; }
    return 1;
}
DRIL_EXPORT int64_t dril_comm_allreduce_calls(const dril_handle* h) { return h ? h->allreduce_calls : -1; }
