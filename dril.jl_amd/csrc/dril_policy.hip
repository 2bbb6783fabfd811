// dril_policy.hip — deployment policies (include/dril_policy.h): the policy object and policy_act_kernel, the one-launch actor
//   normalise -> every Dense layer -> distribution head -> action adapter
// for a small batch of raw observations.  Stands in for src/deployment/deployment_policy.jl (NeuralPolicy, NormWrapperPolicy) of the reference.
//
// policy_act_kernel: one workgroup takes a tile of TC batch columns through the whole net.  Two activation panels [width][TC] ping-pong in LDS; the weights
// stream from global memory (L2-resident after the first call).  A wave owns 64 output rows x 4 columns at a time: lane = output row, so a k-step's weight read is
// one coalesced 256-byte line of the column-major (out x in) matrix, and the 4 activations of that k-step are one broadcast ds_read_b128.  Plain f32 FMA, k ascending,
// one accumulator per (row, column): the arithmetic of a column is the same whatever tile width, tile position or neighbours it has, so an observation's action is
// bit-identical alone and inside any batch.  At these batch sizes a layer is a mat-vec bound by the weight read: no MFMA, no reduced-precision pieces, no range caveat.
// No grid barrier, no cooperative launch, no atomics.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/dril_policy.h"
#include "../../include/device/dril_philox.h"
#include "../../include/device/dril_activations.h"
#include "dril_gemm.h"
#include "dril_policy_internal.h"
#include "dril_sac_adapter.h"

using namespace dril;

#define DRIL_EXPORT extern "C" __attribute__((visibility("default")))

namespace dril {
hipError_t set_max_dynamic_lds(const void* fn, size_t bytes);   // dril_kernels.hip
}

namespace {

constexpr int kMaxLayers = 5;            // 1 - 4 hidden layers + the output layer
constexpr int kActThreads = 1024;        // 16 waves: a [1024]-wide layer is 16 row tiles, one per wave
constexpr int kActWaves = kActThreads / 64;
constexpr int kColsPerThread = 4;
constexpr int kUnroll = 16;              // weight lines a wave keeps in flight
constexpr int64_t kDefaultThreshold = 256;
constexpr int kChunkRows = 4096;         // over-threshold path: rows per pass of the layer contractions

struct PolicyActArgs {
    const float* P;                                                      // the actor net; layer l: W at P + w[l] (out x in, column-major), b at P + b[l]
    int nl, in[kMaxLayers], out[kMaxLayers], w[kMaxLayers], b[kMaxLayers];
    int kind, D, A, act, action_start, has_norm, deterministic, panel;   // panel: floats of one activation panel (max width x TC)
    float clip, eps;
    const float *log_std, *mean, *var, *low, *high;
    const float* obs; const void* noise; long long B;
    void* raw; void* env;
    unsigned long long seed, call;
};

// normalize_obs! (normalizeWrapperEnv.jl:174-179)
__device__ __forceinline__ float policy_normalize(const PolicyActArgs& g, float x, int k) {
    const float v = (x - g.mean[k]) / sqrtf(g.var[k] + g.eps);
    return fminf(fmaxf(v, -g.clip), g.clip);
}
// the policy's own noise: Philox keyed by its seed, counter (row, component block, call)
__device__ __forceinline__ double policy_noise_u01(const PolicyActArgs& g, long long row) {
    uint32_t r[4]; philox4x32_10((uint32_t)g.seed, (uint32_t)(g.seed >> 32), (uint32_t)row, (uint32_t)(row >> 32), 0u, (uint32_t)g.call, r);
    return u01_f64(r[0], r[1]);
}
__device__ __forceinline__ float policy_noise_randn(const PolicyActArgs& g, long long row, int i) {
    uint32_t r[4]; philox4x32_10((uint32_t)g.seed, (uint32_t)(g.seed >> 32), (uint32_t)row, (uint32_t)(row >> 32), 16u + (uint32_t)(i / 2), (uint32_t)g.call, r);
    return (i & 1) ? randn_f32(r[2], r[3]) : randn_f32(r[0], r[1]);
}

// distribution head + adapter of batch row b; z[a * zs]: the output layer's row (logits | means)
__device__ __forceinline__ void policy_head(const PolicyActArgs& g, const float* z, int zs, long long b) {
    const int A = g.A;
    if (g.kind == DRIL_POLICY_CATEGORICAL) {                                         // Lux.softmax + Categorical (layer_forward.jl:141-149, categorical.jl:42-52), as generic_policy_head_kernel
        float m = z[0]; for (int i = 1; i < A; ++i) m = fmaxf(m, z[i * zs]);
        float s = 0.f; for (int i = 0; i < A; ++i) s += expf(z[i * zs] - m);
        int act;
        if (g.deterministic) {                                                       // mode(d) = argmax(p), first maximum
            act = 0; float best = expf(z[0] - m) / s;
            for (int k = 1; k < A; ++k) { const float p = expf(z[k * zs] - m) / s; if (p > best) { best = p; act = k; } }
        } else {
            const double u = g.noise ? ((const double*)g.noise)[b] : policy_noise_u01(g, b);
            float cs = 0.f; act = A - 1;                                              // findfirst(cumsum(p) .>= u)
            for (int k = 0; k < A; ++k) { cs += expf(z[k * zs] - m) / s; if ((double)cs >= u) { act = k; break; } }
        }
        if (g.raw) ((int32_t*)g.raw)[b] = act + g.action_start;                       // DiscreteAdapter: the action as it is
        if (g.env) ((int32_t*)g.env)[b] = act + g.action_start;
        return;
    }
    float* raw = g.raw ? (float*)g.raw + b * A : nullptr;
    float* env = g.env ? (float*)g.env + b * A : nullptr;
    for (int k = 0; k < A; ++k) {
        const float mu = z[k * zs];
        float n01 = 0.f;
        if (!g.deterministic) n01 = g.noise ? ((const float*)g.noise)[b * A + k] : policy_noise_randn(g, b, k);
        const float lo = g.low[k], hi = g.high[k];
        float r, e;
        if (g.kind == DRIL_POLICY_DIAG_GAUSSIAN) {
            r = g.deterministic ? mu : mu + expf(g.log_std[k]) * n01;                 // diagGaussian.jl:13-17, mode(d) = mean :45-47
            e = lo < hi ? fminf(fmaxf(r, lo), hi) : r;                                // to_env(ClampAdapter), default_adapters.jl:4-11
        } else {
            r = tanhf(mu + expf(g.log_std[k]) * n01);                                 // squashedDiagGaussian.jl:24-27, mode(d) = tanh(mean) :48-50
            e = sac_to_env(r, lo, hi);                                                // to_env(TanhScaleAdapter): squashes again, as the reference has it
        }
        if (raw) raw[k] = r;
        if (env) env[k] = e;
    }
}

// rows [o] x NC columns of one Dense layer: acc_j = sum_k W[o][k] x[k][j], k ascending, one FMA per term.  W: the matrix at row o; x: the panel at the unit's first column
template <int NC, int TC>
__device__ __forceinline__ void dense_unit(const float* __restrict__ W, int O, int K, const float* x, float (&acc)[NC]) {
#pragma unroll
    for (int j = 0; j < NC; ++j) acc[j] = 0.f;
    auto term = [&](float w, int k) {
        if constexpr (NC == 4) {
            const float4 v = *(const float4*)(x + k * TC);
            acc[0] = __builtin_fmaf(w, v.x, acc[0]); acc[1] = __builtin_fmaf(w, v.y, acc[1]); acc[2] = __builtin_fmaf(w, v.z, acc[2]); acc[3] = __builtin_fmaf(w, v.w, acc[3]);
        } else acc[0] = __builtin_fmaf(w, x[k * TC], acc[0]);
    };
    int k = 0;
    for (; k + kUnroll <= K; k += kUnroll) {
        float w[kUnroll];
#pragma unroll
        for (int i = 0; i < kUnroll; ++i) w[i] = W[(size_t)(k + i) * O];              // all of the step's lines leave before the first is consumed
#pragma unroll
        for (int i = 0; i < kUnroll; ++i) term(w[i], k + i);
    }
    for (; k < K; ++k) term(W[(size_t)k * O], k);
}

template <int TC>
__global__ __launch_bounds__(kActThreads) void policy_act_kernel(PolicyActArgs g) {
    extern __shared__ float4 policy_lds[];
    float* in = (float*)policy_lds; float* out = in + g.panel;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long c0 = (long long)blockIdx.x * TC;
    const int ncol = (int)(g.B - c0 < TC ? g.B - c0 : TC);
    // the tile's observations, normalised, as panel [k][c]; columns past the batch are zero
    for (int i = tid; i < g.D * TC; i += kActThreads) {
        const int c = i / g.D, k = i - c * g.D;
        float v = 0.f;
        if (c < ncol) { v = g.obs[(c0 + c) * g.D + k]; if (g.has_norm) v = policy_normalize(g, v, k); }
        in[k * TC + c] = v;
    }
    __syncthreads();
    for (int l = 0; l < g.nl; ++l) {
        const int K = g.in[l], O = g.out[l];
        const float* __restrict__ W = g.P + g.w[l]; const float* __restrict__ bias = g.P + g.b[l];
        const int nrt = (O + 63) >> 6, units = nrt * ((ncol + kColsPerThread - 1) / kColsPerThread);
        const bool hidden = l + 1 < g.nl;
        for (int u = wave; u < units; u += kActWaves) {                             // unit = 64 rows x 4 columns; column groups past the batch are not computed
            const int cg = u / nrt, o = (u - cg * nrt) * 64 + lane, cb = cg * kColsPerThread;
            if (o >= O) continue;
            const float bo = bias[o];
            float* dst = out + o * TC + cb;
            if (ncol - cb == 1) {
                float acc[1]; dense_unit<1, TC>(W + o, O, K, in + cb, acc);
                const float v = acc[0] + bo;
                dst[0] = hidden ? activation_forward(g.act, v) : v;
            } else {
                float acc[4]; dense_unit<4, TC>(W + o, O, K, in + cb, acc);
                float4 v;
                v.x = acc[0] + bo; v.y = acc[1] + bo; v.z = acc[2] + bo; v.w = acc[3] + bo;
                if (hidden) { v.x = activation_forward(g.act, v.x); v.y = activation_forward(g.act, v.y); v.z = activation_forward(g.act, v.z); v.w = activation_forward(g.act, v.w); }
                *(float4*)dst = v;
            }
        }
        __syncthreads();
        float* t = in; in = out; out = t;
    }
    if (tid < ncol) policy_head(g, in + tid, TC, c0 + tid);
}

// ---- the over-threshold path: the layer contractions of dril_gemm.h between these two ---------------------------------------------------------------
__global__ void policy_normalize_kernel(PolicyActArgs g, long long r0, long long n, float* x) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * g.D) return;
    x[i] = policy_normalize(g, g.obs[r0 * g.D + i], (int)(i % g.D));
}
__global__ void policy_head_kernel(PolicyActArgs g, long long r0, long long n, const float* z) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) policy_head(g, z + i * g.A, 1, r0 + i);
}

thread_local std::string g_policy_create_error;

template <typename T> void free_dev(T*& p) { if (p) (void)hipFree(p); p = nullptr; }
template <typename T> void free_host(T*& p) { if (p) (void)hipHostFree(p); p = nullptr; }
size_t round16(size_t b) { return (b + 15) & ~(size_t)15; }
int round4i(int x) { return (x + 3) & ~3; }

}  // namespace

struct dril_policy {
    dril_policy_desc desc{};
    int nl = 0, in[kMaxLayers] = {0}, out[kMaxLayers] = {0}, w[kMaxLayers] = {0}, b[kMaxLayers] = {0};
    int n_params = 0, max_width = 0;
    int o_ls = 0, o_mean = 0, o_var = 0, o_low = 0, o_high = 0, blob_floats = 0;   // the device block: [actor | log_std 64 | mean D | var D | low 64 | high 64]
    float* blob = nullptr;
    hipStream_t stream = nullptr;
    uint64_t seed = 0, calls = 0;
    int64_t threshold = kDefaultThreshold;
    char *h_in = nullptr, *h_out = nullptr, *d_in = nullptr, *d_out = nullptr; size_t cap_in = 0, cap_out = 0;   // pinned staging + their device twins
    float* ws = nullptr; size_t ws_cap = 0;                                          // over-threshold path: normalised rows + two activation buffers
    bool timing = false; hipEvent_t ev_a = nullptr, ev_b = nullptr; double last_ms = -1.0;
    std::string err;
};

namespace {

int pfail(dril_policy* p, int code, const std::string& msg) { if (p) p->err = msg; else g_policy_create_error = msg; return code; }
#define PHIP(p, expr)                                                                                        \
    do { hipError_t _e = (expr); if (_e != hipSuccess)                                                       \
        return pfail(p, DRIL_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); } while (0)
#define PNEED(p) do { if (!(p)) return pfail(nullptr, DRIL_ERR_NOT_INITIALISED, "null policy"); (void)hipSetDevice((p)->desc.device); } while (0)

bool is_box(int kind) { return kind != DRIL_POLICY_CATEGORICAL; }

// the descriptor's checks (no device needed): "" when it is a policy the library can run
std::string check_desc(const dril_policy_desc& d) {
    if (d.abi_version != DRIL_POLICY_ABI_VERSION) return "abi_version mismatch";
    if (d.kind < DRIL_POLICY_CATEGORICAL || d.kind > DRIL_POLICY_SQUASHED_DIAG_GAUSSIAN) return "kind must be 0 (Categorical), 1 (DiagGaussian) or 2 (SquashedDiagGaussian)";
    if (d.obs_dim < 1 || d.obs_dim > DRIL_POLICY_MAX_WIDTH) return "obs_dim must be 1..1024";
    if (d.action_dim < 1 || d.action_dim > DRIL_POLICY_MAX_ACTION_DIM) return "action_dim must be 1..64";
    if (d.n_hidden < 1 || d.n_hidden > 4) return "n_hidden must be 1..4";
    for (int l = 0; l < d.n_hidden; ++l) if (d.hidden[l] < 1 || d.hidden[l] > DRIL_POLICY_MAX_WIDTH) return "hidden widths must be 1..1024";
    if (d.activation < 0 || d.activation > 7) return "activation must be 0 (tanh), 1 (relu), 2 (sigmoid), 3 (elu), 4 (leakyrelu), 5 (softplus), 6 (gelu) or 7 (swish)";
    if (d.has_norm && !(d.clip_obs > 0.f)) return "has_norm: clip_obs must be positive";
    if (d.has_norm && !(d.epsilon >= 0.f)) return "has_norm: epsilon must not be negative";
    if (d.device < 0) return "device must not be negative";
    return "";
}
size_t desc_param_count(const dril_policy_desc& d) {
    size_t n = 0; int in = d.obs_dim;
    for (int l = 0; l <= d.n_hidden; ++l) { const int out = l == d.n_hidden ? d.action_dim : d.hidden[l]; n += (size_t)in * out + out; in = out; }
    return n;
}

void policy_free(dril_policy* p) {
    if (!p) return;
    (void)hipSetDevice(p->desc.device);
    if (p->stream) (void)hipStreamSynchronize(p->stream);
    free_dev(p->blob); free_dev(p->d_in); free_dev(p->d_out); free_dev(p->ws); free_host(p->h_in); free_host(p->h_out);
    if (p->ev_a) (void)hipEventDestroy(p->ev_a); if (p->ev_b) (void)hipEventDestroy(p->ev_b);
    if (p->stream) (void)hipStreamDestroy(p->stream);
    delete p;
}

// the object with its device block holding everything the descriptor gives (bounds; log_std 0, mean 0, var 1 until the caller fills them); *blob_host is that block
int policy_alloc(const dril_policy_desc& d, dril_policy** out, std::vector<float>* blob_host) {
    const std::string bad = check_desc(d);
    if (!bad.empty()) return pfail(nullptr, DRIL_ERR_INVALID_ARG, bad);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || d.device >= ndev) return pfail(nullptr, DRIL_ERR_HIP, "no such device");
    PHIP(nullptr, hipSetDevice(d.device));
    hipDeviceProp_t prop; PHIP(nullptr, hipGetDeviceProperties(&prop, d.device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return pfail(nullptr, DRIL_ERR_UNSUPPORTED, std::string("libdril_hip targets gfx950 (MI355X) only; device is ") + prop.gcnArchName);
    dril_policy* p = nullptr;
    try { p = new dril_policy(); } catch (...) { return pfail(nullptr, DRIL_ERR_INVALID_ARG, "out of host memory"); }
    p->desc = d; p->desc.reserved = 0;
    if (!is_box(d.kind)) { std::memset(p->desc.action_low, 0, sizeof(p->desc.action_low)); std::memset(p->desc.action_high, 0, sizeof(p->desc.action_high)); }
    else p->desc.action_start = 0;
    for (int l = d.n_hidden; l < 4; ++l) p->desc.hidden[l] = 0;
    p->nl = d.n_hidden + 1; p->max_width = std::max(d.obs_dim, d.action_dim);
    int off = 0;
    for (int l = 0; l < p->nl; ++l) {
        p->in[l] = l == 0 ? d.obs_dim : d.hidden[l - 1]; p->out[l] = l == d.n_hidden ? d.action_dim : d.hidden[l];
        p->w[l] = off; off += p->in[l] * p->out[l]; p->b[l] = off; off += p->out[l];
        p->max_width = std::max(p->max_width, p->out[l]);
    }
    p->n_params = off;
    p->o_ls = round4i(off); p->o_mean = p->o_ls + DRIL_POLICY_MAX_ACTION_DIM; p->o_var = p->o_mean + round4i(d.obs_dim); p->o_low = p->o_var + round4i(d.obs_dim);
    p->o_high = p->o_low + DRIL_POLICY_MAX_ACTION_DIM; p->blob_floats = p->o_high + DRIL_POLICY_MAX_ACTION_DIM;
    blob_host->assign((size_t)p->blob_floats, 0.f);
    for (int k = 0; k < d.obs_dim; ++k) (*blob_host)[p->o_var + k] = 1.0f;
    std::memcpy(blob_host->data() + p->o_low, p->desc.action_low, sizeof(p->desc.action_low)); std::memcpy(blob_host->data() + p->o_high, p->desc.action_high, sizeof(p->desc.action_high));
    hipError_t e = hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipMalloc((void**)&p->blob, (size_t)p->blob_floats * 4);
    if (e != hipSuccess) { policy_free(p); return pfail(nullptr, DRIL_ERR_HIP, std::string("policy allocation: ") + hipGetErrorString(e)); }
    *out = p;
    return DRIL_OK;
}

PolicyActArgs act_args(const dril_policy* p) {
    PolicyActArgs g{};
    g.P = p->blob; g.nl = p->nl;
    for (int l = 0; l < p->nl; ++l) { g.in[l] = p->in[l]; g.out[l] = p->out[l]; g.w[l] = p->w[l]; g.b[l] = p->b[l]; }
    g.kind = p->desc.kind; g.D = p->desc.obs_dim; g.A = p->desc.action_dim; g.act = p->desc.activation; g.action_start = p->desc.action_start; g.has_norm = p->desc.has_norm;
    g.clip = p->desc.clip_obs; g.eps = p->desc.epsilon;
    g.log_std = p->blob + p->o_ls; g.mean = p->blob + p->o_mean; g.var = p->blob + p->o_var; g.low = p->blob + p->o_low; g.high = p->blob + p->o_high;
    g.seed = p->seed; g.call = p->calls;
    return g;
}

template <int TC> hipError_t launch_act(const dril_policy* p, PolicyActArgs g, hipStream_t s) {
    g.panel = p->max_width * TC;
    const size_t lds = 2 * (size_t)g.panel * sizeof(float);                           // 128 KB at width 1024 and TC 16: inside the 160 KB of a gfx950 CU
    if (lds > 64 * 1024) { hipError_t e = set_max_dynamic_lds((const void*)policy_act_kernel<TC>, lds); if (e != hipSuccess) return e; }
    const unsigned blocks = (unsigned)((g.B + TC - 1) / TC);
    hipLaunchKernelGGL(policy_act_kernel<TC>, dim3(blocks), dim3(kActThreads), lds, s, g);
    return hipGetLastError();
}
// up to the default threshold in tiles of 4 columns (more workgroups, each a quarter of the FMA work: a tile's time is its FMA count once the weights are in L2), larger
// batches in tiles of 16 (a quarter of the weight traffic): the tile width changes no result
hipError_t run_kernel_path(const dril_policy* p, const PolicyActArgs& g, hipStream_t s) { return g.B <= kDefaultThreshold ? launch_act<4>(p, g, s) : launch_act<16>(p, g, s); }

hipError_t run_gemm_path(dril_policy* p, const PolicyActArgs& g0, hipStream_t s) {
    const size_t rows = (size_t)std::min<long long>(kChunkRows, g0.B), need = rows * ((size_t)round4i(g0.D) + 2 * (size_t)round4i(p->max_width));
    if (need > p->ws_cap) {
        free_dev(p->ws); p->ws_cap = 0;
        hipError_t e = hipMalloc((void**)&p->ws, need * 4); if (e != hipSuccess) return e;
        p->ws_cap = need;
    }
    float* xn = p->ws; float* bufs[2] = {xn + rows * round4i(g0.D), xn + rows * ((size_t)round4i(g0.D) + round4i(p->max_width))};
    const int epi = epi_of_activation(g0.act);
    for (long long r0 = 0; r0 < g0.B; r0 += kChunkRows) {
        const long long n = std::min<long long>(kChunkRows, g0.B - r0);
        const float* x = g0.obs + r0 * g0.D;
        if (g0.has_norm) {
            hipLaunchKernelGGL(policy_normalize_kernel, dim3((unsigned)((n * g0.D + 255) / 256)), dim3(256), 0, s, g0, r0, n, xn);
            hipError_t e = hipGetLastError(); if (e != hipSuccess) return e;
            x = xn;
        }
        for (int l = 0; l < g0.nl; ++l) {                                            // y = act(W x + b), as mlp_forward of the generic on-policy path; f32 MFMA (no operand split)
            GemmArgs a = gemm_args();
            a.A = g0.P + g0.w[l]; a.sAm = 1; a.sAk = g0.out[l]; a.B = x; a.sBk = 1; a.sBn = g0.in[l]; a.C = bufs[l & 1]; a.sCm = 1; a.sCn = g0.out[l]; a.bias = g0.P + g0.b[l];
            a.M = g0.out[l]; a.N = (int)n; a.K = g0.in[l]; a.epi = l + 1 < g0.nl ? epi : EPI_NONE;
            hipError_t e = launch_gemm(a, 1, s); if (e != hipSuccess) return e;
            x = bufs[l & 1];
        }
        hipLaunchKernelGGL(policy_head_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, g0, r0, n, x);
        hipError_t e = hipGetLastError(); if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

int grow(dril_policy* p, char*& host, char*& dev, size_t& cap, size_t need) {
    if (need <= cap) return DRIL_OK;
    PHIP(p, hipStreamSynchronize(p->stream));
    free_host(host); free_dev(dev); cap = 0;
    const size_t want = std::max<size_t>(4096, need + need / 2);
    PHIP(p, hipHostMalloc((void**)&host, want)); PHIP(p, hipMalloc((void**)&dev, want));
    cap = want;
    return DRIL_OK;
}

}  // namespace

namespace dril {

void policy_set_create_error(const std::string& msg) { g_policy_create_error = msg; }

int policy_from_device(const PolicyDeviceSource& src, dril_policy** out, std::string* msg) {
    auto bad = [&](int code, const std::string& m) { *msg = m; g_policy_create_error = m; return code; };
    if (!out) return bad(DRIL_ERR_INVALID_ARG, "null out pointer");
    *out = nullptr;
    if (!src.actor || src.n != desc_param_count(src.desc)) return bad(DRIL_ERR_INVALID_ARG, "the handle's actor does not have the parameter count its shape implies");
    dril_policy* p = nullptr; std::vector<float> host;
    const int rc = policy_alloc(src.desc, &p, &host);
    if (rc) { *msg = g_policy_create_error; return rc; }
    hipError_t e = hipMemcpy(p->blob, host.data(), host.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpyAsync(p->blob, src.actor, src.n * 4, hipMemcpyDeviceToDevice, src.stream);
    if (e == hipSuccess && is_box(src.desc.kind)) e = src.log_std ? hipMemcpyAsync(p->blob + p->o_ls, src.log_std, (size_t)src.desc.action_dim * 4, hipMemcpyDeviceToDevice, src.stream) : hipErrorInvalidValue;
    if (e == hipSuccess && src.desc.has_norm) {
        e = (src.obs_mean && src.obs_var) ? hipMemcpyAsync(p->blob + p->o_mean, src.obs_mean, (size_t)src.desc.obs_dim * 4, hipMemcpyDeviceToDevice, src.stream) : hipErrorInvalidValue;
        if (e == hipSuccess) e = hipMemcpyAsync(p->blob + p->o_var, src.obs_var, (size_t)src.desc.obs_dim * 4, hipMemcpyDeviceToDevice, src.stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(src.stream);
    if (e != hipSuccess) { policy_free(p); return bad(DRIL_ERR_HIP, std::string("policy snapshot: ") + hipGetErrorString(e)); }
    *out = p;
    return DRIL_OK;
}

}  // namespace dril

DRIL_EXPORT int32_t dril_policy_create(const dril_policy_desc* desc, const float* actor_params, size_t n, const float* log_std, const float* obs_mean, const float* obs_var,
                                       dril_policy** out) {
    if (!desc || !out) return pfail(nullptr, DRIL_ERR_INVALID_ARG, "dril_policy_create: null desc / out");
    *out = nullptr;
    { const std::string bad = check_desc(*desc); if (!bad.empty()) return pfail(nullptr, DRIL_ERR_INVALID_ARG, "dril_policy_create: " + bad); }
    if (!actor_params) return pfail(nullptr, DRIL_ERR_INVALID_ARG, "dril_policy_create: null actor_params");
    if (n != desc_param_count(*desc)) return pfail(nullptr, DRIL_ERR_INVALID_ARG, "dril_policy_create: n = " + std::to_string(n) + " but the descriptor's actor has " + std::to_string(desc_param_count(*desc)) + " parameters");
    if (is_box(desc->kind) && !log_std) return pfail(nullptr, DRIL_ERR_INVALID_ARG, "dril_policy_create: the Gaussian kinds need log_std");
    if (desc->has_norm && (!obs_mean || !obs_var)) return pfail(nullptr, DRIL_ERR_INVALID_ARG, "dril_policy_create: has_norm needs obs_mean and obs_var");
    dril_policy* p = nullptr; std::vector<float> host;
    const int rc = policy_alloc(*desc, &p, &host); if (rc) return rc;
    std::memcpy(host.data(), actor_params, n * 4);
    if (is_box(desc->kind)) std::memcpy(host.data() + p->o_ls, log_std, (size_t)desc->action_dim * 4);
    if (desc->has_norm) { std::memcpy(host.data() + p->o_mean, obs_mean, (size_t)desc->obs_dim * 4); std::memcpy(host.data() + p->o_var, obs_var, (size_t)desc->obs_dim * 4); }
    const hipError_t e = hipMemcpy(p->blob, host.data(), host.size() * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) { policy_free(p); return pfail(nullptr, DRIL_ERR_HIP, std::string("dril_policy_create: ") + hipGetErrorString(e)); }
    *out = p;
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_policy_destroy(dril_policy* p) {
    if (!p) return pfail(nullptr, DRIL_ERR_NOT_INITIALISED, "null policy");
    policy_free(p);
    return DRIL_OK;
}
DRIL_EXPORT const char* dril_policy_last_error(const dril_policy* p) { return p ? p->err.c_str() : g_policy_create_error.c_str(); }

DRIL_EXPORT int32_t dril_policy_act(dril_policy* p, const float* obs, int64_t batch, int32_t deterministic, const void* noise, void* raw_actions, void* env_actions) {
    PNEED(p);
    if (!obs) return pfail(p, DRIL_ERR_INVALID_ARG, "dril_policy_act: null obs");
    if (batch < 1 || batch > (int64_t)1 << 30) return pfail(p, DRIL_ERR_INVALID_ARG, "dril_policy_act: batch must be 1 .. 2^30");
    if (!raw_actions && !env_actions) return pfail(p, DRIL_ERR_INVALID_ARG, "dril_policy_act: both output pointers are null");
    const dril_policy_desc& d = p->desc;
    const bool box = is_box(d.kind);
    if (deterministic) noise = nullptr;
    const size_t nb = noise ? (size_t)batch * (box ? 4 * (size_t)d.action_dim : 8) : 0, obs_off = round16(nb), in_bytes = obs_off + (size_t)batch * d.obs_dim * 4;
    const size_t ab = (size_t)batch * (box ? 4 * (size_t)d.action_dim : 4), env_off = round16(ab), out_bytes = env_off + ab;
    { int rc = grow(p, p->h_in, p->d_in, p->cap_in, in_bytes); if (rc) return rc; }
    { int rc = grow(p, p->h_out, p->d_out, p->cap_out, out_bytes); if (rc) return rc; }
    if (noise) std::memcpy(p->h_in, noise, nb);
    std::memcpy(p->h_in + obs_off, obs, (size_t)batch * d.obs_dim * 4);
    PHIP(p, hipMemcpyAsync(p->d_in, p->h_in, in_bytes, hipMemcpyHostToDevice, p->stream));
    PolicyActArgs g = act_args(p);
    g.obs = (const float*)(p->d_in + obs_off); g.noise = noise ? (const void*)p->d_in : nullptr; g.B = batch; g.deterministic = deterministic ? 1 : 0;
    g.raw = raw_actions ? (void*)p->d_out : nullptr; g.env = env_actions ? (void*)(p->d_out + env_off) : nullptr;
    if (!deterministic && !noise) p->calls += 1;                                     // the next sampling call draws from the next block of the stream
    if (p->timing) PHIP(p, hipEventRecord(p->ev_a, p->stream));
    PHIP(p, batch <= p->threshold ? run_kernel_path(p, g, p->stream) : run_gemm_path(p, g, p->stream));
    if (p->timing) PHIP(p, hipEventRecord(p->ev_b, p->stream));
    const size_t o0 = raw_actions ? 0 : env_off, o1 = env_actions ? out_bytes : ab;   // one copy spanning what was asked for
    PHIP(p, hipMemcpyAsync(p->h_out + o0, p->d_out + o0, o1 - o0, hipMemcpyDeviceToHost, p->stream));
    PHIP(p, hipStreamSynchronize(p->stream));
    if (raw_actions) std::memcpy(raw_actions, p->h_out, ab);
    if (env_actions) std::memcpy(env_actions, p->h_out + env_off, ab);
    if (p->timing) { float ms = 0.f; if (hipEventElapsedTime(&ms, p->ev_a, p->ev_b) == hipSuccess) p->last_ms = ms; }
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_policy_set_seed(dril_policy* p, uint64_t seed) { PNEED(p); p->seed = seed; p->calls = 0; return DRIL_OK; }
DRIL_EXPORT int32_t dril_policy_set_threshold(dril_policy* p, int64_t threshold) { PNEED(p); p->threshold = threshold > 0 ? threshold : kDefaultThreshold; return DRIL_OK; }
DRIL_EXPORT int32_t dril_policy_kernel_time(dril_policy* p, int32_t enable, double* last_ms) {
    PNEED(p);
    if (enable && !p->ev_a) { PHIP(p, hipEventCreate(&p->ev_a)); PHIP(p, hipEventCreate(&p->ev_b)); }
    p->timing = enable != 0;
    if (last_ms) *last_ms = p->last_ms;
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_policy_describe(const dril_policy* p, dril_policy_desc* out) {
    if (!p) return pfail(nullptr, DRIL_ERR_NOT_INITIALISED, "null policy");
    if (!out) return pfail(const_cast<dril_policy*>(p), DRIL_ERR_INVALID_ARG, "dril_policy_describe: null out pointer");
    *out = p->desc;
    return DRIL_OK;
}
DRIL_EXPORT int64_t dril_policy_param_count(const dril_policy* p) { return p ? p->n_params : -1; }
DRIL_EXPORT int32_t dril_policy_get_params(dril_policy* p, float* actor_params, size_t n, float* log_std) {
    PNEED(p);
    if (!actor_params || n != (size_t)p->n_params) return pfail(p, DRIL_ERR_INVALID_ARG, "dril_policy_get_params: n must equal dril_policy_param_count");
    PHIP(p, hipMemcpy(actor_params, p->blob, n * 4, hipMemcpyDeviceToHost));
    if (log_std && is_box(p->desc.kind)) PHIP(p, hipMemcpy(log_std, p->blob + p->o_ls, (size_t)p->desc.action_dim * 4, hipMemcpyDeviceToHost));
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_policy_get_norm(dril_policy* p, float* obs_mean, float* obs_var) {
    PNEED(p);
    if (!p->desc.has_norm) return pfail(p, DRIL_ERR_NOT_INITIALISED, "dril_policy_get_norm: the policy carries no observation statistics (a plain NeuralPolicy)");
    if (!obs_mean || !obs_var) return pfail(p, DRIL_ERR_INVALID_ARG, "dril_policy_get_norm: null out pointer");
    PHIP(p, hipMemcpy(obs_mean, p->blob + p->o_mean, (size_t)p->desc.obs_dim * 4, hipMemcpyDeviceToHost));
    PHIP(p, hipMemcpy(obs_var, p->blob + p->o_var, (size_t)p->desc.obs_dim * 4, hipMemcpyDeviceToHost));
    return DRIL_OK;
}
