// dril_env_side.h — the env side of a handle: the envs a PPO handle (dril_handle.h) or a SAC handle (dril_sac_handle.h) steps on the device, whichever they are — a built-in
// kind (dril_env_kinds.h; the env kernels of dril_kernels.hip) or a device env plug-in (include/device/dril_env_plugin.h; a HIP module loaded at create).  The ONE
// definition of loading a plug-in (path checks, descriptor checks, load order), of the argument block its kernels take, and of reset! / observe / act! over either.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/dril_hip.h"
#include "../../include/device/dril_env_plugin.h"   // DrilEnvPluginDesc / DrilEnvPluginArgs: the same definitions a plug-in is compiled with
#include "../../include/device/dril_env_world.h"    // the limits of a world (N agents per state): descriptor word `agents`
#include "../../include/device/dril_env_rollout.h"  // DrilEnvRolloutDesc / DrilEnvRolloutArgs: the fused rollout a plug-in may carry
#include "../../include/device/dril_env_rollout_pop.h"  // DrilEnvRolloutPopDesc: the population entry of the fused rollout a plug-in may carry
#include "../../include/device/dril_env_evaluate.h" // DrilEnvEvaluateDesc / DrilEnvEvaluateArgs: the fused evaluation a plug-in may carry
#include "dril_internal.h"

namespace dril {
// ---- loading a device env plug-in ----
// the checks that need no GPU: a path, a readable file, the magic of a code object (ELF, or the clang-offload-bundle hipcc writes without --no-gpu-bundle-output)
inline int check_code_object_path(const char* path, std::string& msg) {
    if (!path || !*path) { msg = "null code_object_path"; return DRIL_ERR_INVALID_ARG; }
    FILE* f = std::fopen(path, "rb");
    if (!f) { msg = std::string("cannot read code object ") + path; return DRIL_ERR_INVALID_ARG; }
    char magic[24] = {0}; const size_t n = std::fread(magic, 1, sizeof(magic), f); std::fclose(f);
    const bool elf = n >= 4 && std::memcmp(magic, "\x7f" "ELF", 4) == 0, bundle = n >= 24 && std::memcmp(magic, "__CLANG_OFFLOAD_BUNDLE__", 24) == 0;
    if (!elf && !bundle) { msg = std::string(path) + " is not a code object (neither an ELF nor a clang-offload-bundle): build it with hipcc --genco --offload-arch=gfx950"; return DRIL_ERR_INVALID_ARG; }
    return DRIL_OK;
}
inline int check_plugin_desc(const DrilEnvPluginDesc& d, std::string& msg) {
    if (d.abi_version != DRIL_ENV_PLUGIN_ABI) { msg = "env plug-in ABI " + std::to_string(d.abi_version) + ", this library speaks " + std::to_string(DRIL_ENV_PLUGIN_ABI) + ": recompile the plug-in against this library's include/device/dril_env_plugin.h"; return DRIL_ERR_UNSUPPORTED; }
    if (d.args_size != sizeof(DrilEnvPluginArgs)) { msg = "env plug-in kernel argument block is " + std::to_string(d.args_size) + " bytes, this library passes " + std::to_string(sizeof(DrilEnvPluginArgs)) + ": recompile the plug-in against this library's include/device/dril_env_plugin.h"; return DRIL_ERR_UNSUPPORTED; }
    // agents: 0 = one env per row (DRIL_ENV_PLUGIN), 2..16 = a world of that many agents per state (DRIL_ENV_PLUGIN_WORLD); a world's S is per world, up to 256
    const bool world = d.agents != 0;
    if (world && (d.agents < DRIL_ENV_WORLD_MIN_N || d.agents > DRIL_ENV_WORLD_MAX_N)) { msg = "env plug-in descriptor out of range: agents " + std::to_string(d.agents) + " (0 for an env, 2..16 for a world)"; return DRIL_ERR_UNSUPPORTED; }
    const int max_s = world ? DRIL_ENV_WORLD_MAX_S : DRIL_ENV_PLUGIN_MAX_S;
    if (d.S < 1 || d.S > max_s || d.D < 1 || d.D > DRIL_ENV_PLUGIN_MAX_D || d.A < 1 || d.A > DRIL_ENV_PLUGIN_MAX_A || d.episode_len < 1) {
        msg = "env plug-in descriptor out of range: S " + std::to_string(d.S) + (world ? " (1..256 per world)" : " (1..64)") + ", D " + std::to_string(d.D) + " (1..1024), A " + std::to_string(d.A) + " (1..64), episode_len " + std::to_string(d.episode_len) + " (>= 1)"; return DRIL_ERR_UNSUPPORTED; }
    return DRIL_OK;
}
// path checks -> hipModuleLoad -> descriptor out and checked; on success the caller owns *mod (nothing of the module has been launched)
inline int load_env_module(const char* path, int device, hipModule_t* mod, DrilEnvPluginDesc* desc, std::string& msg) {
    *mod = nullptr;
    int rc = check_code_object_path(path, msg); if (rc) return rc;
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) { msg = std::string("hipSetDevice: ") + hipGetErrorString(e); return DRIL_ERR_HIP; }
    e = hipModuleLoad(mod, path);
    if (e != hipSuccess) { *mod = nullptr; (void)hipGetLastError(); msg = std::string("hipModuleLoad(") + path + "): " + hipGetErrorString(e) + " (a code object for gfx950 is needed)"; return DRIL_ERR_HIP; }
    hipDeviceptr_t dptr = nullptr; size_t bytes = 0;
    e = hipModuleGetGlobal(&dptr, &bytes, *mod, "dril_env_plugin_desc");
    if (e != hipSuccess) { msg = std::string(path) + " has no symbol dril_env_plugin_desc (not built with DRIL_ENV_PLUGIN): " + hipGetErrorString(e); rc = DRIL_ERR_UNSUPPORTED; }
    else if (bytes != sizeof(DrilEnvPluginDesc)) { msg = std::string(path) + ": dril_env_plugin_desc is " + std::to_string(bytes) + " bytes, this library reads " + std::to_string(sizeof(DrilEnvPluginDesc)) + " (another plug-in ABI)"; rc = DRIL_ERR_UNSUPPORTED; }
    else {
        e = hipMemcpy(desc, dptr, sizeof(*desc), hipMemcpyDeviceToHost);
        if (e != hipSuccess) { msg = std::string("copying dril_env_plugin_desc: ") + hipGetErrorString(e); rc = DRIL_ERR_HIP; }
        else { desc->name[sizeof(desc->name) - 1] = 0; rc = check_plugin_desc(*desc, msg); }
    }
    if (rc) { (void)hipModuleUnload(*mod); *mod = nullptr; (void)hipGetLastError(); }   // (a refused module must not leave its error behind: the launchers read hipGetLastError after their launches)
    return rc;
}
inline void fill_module_info(const DrilEnvPluginDesc& d, dril_env_module_info* o) {
    std::memset(o, 0, sizeof(*o));
    o->plugin_abi = d.abi_version; o->state_dim = d.S; o->obs_dim = d.D; o->action_dim = d.A; o->discrete = d.discrete ? 1 : 0; o->episode_len = d.episode_len;
    static_assert(sizeof(o->action_low) == sizeof(d.action_low) && sizeof(o->name) == sizeof(d.name), "dril_env_module_info mirrors DrilEnvPluginDesc");
    std::memcpy(o->action_low, d.action_low, sizeof(d.action_low)); std::memcpy(o->action_high, d.action_high, sizeof(d.action_high)); std::memcpy(o->name, d.name, sizeof(d.name));
}
// one of the module's three kernels over a.E envs: ceil(E / 256) workgroups of 256 threads, one thread per env (the kernels check e < E)
inline hipError_t env_module_launch(hipFunction_t f, DrilEnvPluginArgs a, hipStream_t stream) {
    void* params[] = {&a};
    return hipModuleLaunchKernel(f, (unsigned)((a.E + DRIL_ENV_PLUGIN_BLOCK - 1) / DRIL_ENV_PLUGIN_BLOCK), 1, 1, DRIL_ENV_PLUGIN_BLOCK, 1, 1, 0, stream, params, nullptr);
}
// the optional entry points of a plug-in (an env that declares obs_low / obs_high): absent ones are null, and asking for one leaves no HIP error behind
inline hipFunction_t env_module_optional(hipModule_t mod, const char* name) {
    hipFunction_t f = nullptr;
    if (hipModuleGetFunction(&f, mod, name) != hipSuccess) { f = nullptr; (void)hipGetLastError(); }
    return f;
}
// The fused rollout of a loaded, checked plug-in (DRIL_ENV_PLUGIN_ROLLOUT, include/device/dril_env_rollout.h): its two kernels and its descriptor, all optional.
// `reason` is empty when the kernel can be launched; a code object without it, or with a descriptor of another ABI number / argument-block size, loads as before
// and says here why the fused path is not available.  Nothing of the module is launched.
struct EnvModuleRollout { hipFunction_t fn = nullptr, fn_scaled = nullptr; DrilEnvRolloutDesc desc{}; bool has_desc = false; std::string reason; };
inline EnvModuleRollout find_module_rollout(hipModule_t mod) {
    EnvModuleRollout r;
    r.fn = env_module_optional(mod, "dril_env_plugin_rollout"); r.fn_scaled = env_module_optional(mod, "dril_env_plugin_rollout_scaled");
    hipDeviceptr_t dptr = nullptr; size_t bytes = 0;
    if (hipModuleGetGlobal(&dptr, &bytes, mod, "dril_env_plugin_rollout_desc") != hipSuccess) { (void)hipGetLastError(); dptr = nullptr; }
    if (!r.fn || !dptr) { r.fn = r.fn_scaled = nullptr; r.reason = "the code object has no fused rollout kernel (dril_env_plugin_rollout): add #include \"device/dril_env_rollout.h\" and DRIL_ENV_PLUGIN_ROLLOUT(Env) to the plug-in's source and rebuild"; return r; }
    if (bytes != sizeof(DrilEnvRolloutDesc) || hipMemcpy(&r.desc, dptr, sizeof(r.desc), hipMemcpyDeviceToHost) != hipSuccess) {
        (void)hipGetLastError(); r.fn = r.fn_scaled = nullptr;
        r.reason = "dril_env_plugin_rollout_desc is " + std::to_string(bytes) + " bytes, this library reads " + std::to_string(sizeof(DrilEnvRolloutDesc)) + ": rebuild the plug-in against this library's include/device/dril_env_rollout.h"; return r; }
    r.has_desc = true;
    if (r.desc.abi_version != DRIL_ENV_ROLLOUT_ABI) r.reason = "fused rollout ABI " + std::to_string(r.desc.abi_version) + ", this library speaks " + std::to_string(DRIL_ENV_ROLLOUT_ABI) + ": rebuild the plug-in against this library's include/device/dril_env_rollout.h";
    else if (r.desc.args_size != sizeof(DrilEnvRolloutArgs)) r.reason = "the fused rollout's argument block is " + std::to_string(r.desc.args_size) + " bytes, this library passes " + std::to_string(sizeof(DrilEnvRolloutArgs)) + ": rebuild the plug-in against this library's include/device/dril_env_rollout.h";
    else if (r.desc.tile < 1 || r.desc.threads < r.desc.tile || r.desc.threads > 1024 || r.desc.max_width < 1) r.reason = "the fused rollout's descriptor is out of range (tile " + std::to_string(r.desc.tile) + ", threads " + std::to_string(r.desc.threads) + ", max width " + std::to_string(r.desc.max_width) + ")";
    if (!r.reason.empty()) r.fn = r.fn_scaled = nullptr;
    return r;
}
// The population entry of the fused rollout (DRIL_ENV_PLUGIN_ROLLOUT_POP, include/device/dril_env_rollout_pop.h), looked up like the rollout itself: two kernels and a
// descriptor, all optional; `reason` is empty when the kernel can be launched, else it names the header and the macro.  Nothing of the module is launched.
struct EnvModuleRolloutPop { hipFunction_t fn = nullptr, fn_scaled = nullptr; DrilEnvRolloutPopDesc desc{}; bool has_desc = false; std::string reason; };
inline EnvModuleRolloutPop find_module_rollout_pop(hipModule_t mod) {
    EnvModuleRolloutPop r;
    r.fn = env_module_optional(mod, "dril_env_plugin_rollout_pop"); r.fn_scaled = env_module_optional(mod, "dril_env_plugin_rollout_pop_scaled");
    hipDeviceptr_t dptr = nullptr; size_t bytes = 0;
    if (hipModuleGetGlobal(&dptr, &bytes, mod, "dril_env_plugin_rollout_pop_desc") != hipSuccess) { (void)hipGetLastError(); dptr = nullptr; }
    const std::string rebuild = ": rebuild the plug-in against this library's include/device/dril_env_rollout_pop.h";
    if (!r.fn || !dptr) { r.fn = r.fn_scaled = nullptr; r.reason = "the code object has no population entry of the fused rollout (dril_env_plugin_rollout_pop): add #include \"device/dril_env_rollout_pop.h\" and DRIL_ENV_PLUGIN_ROLLOUT_POP(Env) after DRIL_ENV_PLUGIN_ROLLOUT(Env) to the plug-in's source and rebuild"; return r; }
    if (bytes != sizeof(DrilEnvRolloutPopDesc) || hipMemcpy(&r.desc, dptr, sizeof(r.desc), hipMemcpyDeviceToHost) != hipSuccess) {
        (void)hipGetLastError(); r.fn = r.fn_scaled = nullptr;
        r.reason = "dril_env_plugin_rollout_pop_desc is " + std::to_string(bytes) + " bytes, this library reads " + std::to_string(sizeof(DrilEnvRolloutPopDesc)) + rebuild; return r; }
    r.has_desc = true;
    if (r.desc.abi_version != DRIL_ENV_ROLLOUT_POP_ABI) r.reason = "population rollout ABI " + std::to_string(r.desc.abi_version) + ", this library speaks " + std::to_string(DRIL_ENV_ROLLOUT_POP_ABI) + rebuild;
    else if (r.desc.args_size != sizeof(DrilEnvRolloutArgs)) r.reason = "a member's block of the population rollout is " + std::to_string(r.desc.args_size) + " bytes, this library passes " + std::to_string(sizeof(DrilEnvRolloutArgs)) + rebuild;
    else if (r.desc.tile < 1 || r.desc.threads < r.desc.tile || r.desc.threads > 1024 || r.desc.max_width < 1) r.reason = "the population rollout's descriptor is out of range (tile " + std::to_string(r.desc.tile) + ", threads " + std::to_string(r.desc.threads) + ", max width " + std::to_string(r.desc.max_width) + ")";
    else if ((r.desc.has_scaled != 0) != (r.fn_scaled != nullptr)) r.reason = std::string("the population rollout's descriptor says has_scaled = ") + std::to_string(r.desc.has_scaled) + ", but dril_env_plugin_rollout_pop_scaled is " + (r.fn_scaled ? "present" : "absent");
    if (!r.reason.empty()) r.fn = r.fn_scaled = nullptr;
    return r;
}
// size and 64-bit FNV-1a hash of a code object file's bytes: what tells two handles' plug-ins apart (a population's members run ONE member's kernel)
inline bool hash_code_object(const char* path, uint64_t* size, uint64_t* hash) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    uint64_t h = 1469598103934665603ull, n = 0; unsigned char buf[4096]; size_t got;
    while ((got = std::fread(buf, 1, sizeof(buf), f)) > 0) { n += got; for (size_t i = 0; i < got; ++i) { h ^= buf[i]; h *= 1099511628211ull; } }
    std::fclose(f);
    *size = n; *hash = h;
    return true;
}
// The fused evaluation of a loaded, checked plug-in (DRIL_ENV_PLUGIN_EVALUATE, include/device/dril_env_evaluate.h), looked up like the rollout: two kernels and a
// descriptor, all optional; `reason` is empty when the kernel can be launched.  Nothing of the module is launched.
struct EnvModuleEvaluate { hipFunction_t fn = nullptr, fn_scaled = nullptr; DrilEnvEvaluateDesc desc{}; bool has_desc = false; std::string reason; };
inline EnvModuleEvaluate find_module_evaluate(hipModule_t mod) {
    EnvModuleEvaluate r;
    r.fn = env_module_optional(mod, "dril_env_plugin_evaluate"); r.fn_scaled = env_module_optional(mod, "dril_env_plugin_evaluate_scaled");
    hipDeviceptr_t dptr = nullptr; size_t bytes = 0;
    if (hipModuleGetGlobal(&dptr, &bytes, mod, "dril_env_plugin_evaluate_desc") != hipSuccess) { (void)hipGetLastError(); dptr = nullptr; }
    const std::string rebuild = ": rebuild the plug-in against this library's include/device/dril_env_evaluate.h";
    if (!r.fn || !dptr) { r.fn = r.fn_scaled = nullptr; r.reason = "the code object has no fused evaluation kernel (dril_env_plugin_evaluate): add #include \"device/dril_env_evaluate.h\" and DRIL_ENV_PLUGIN_EVALUATE(Env) to the plug-in's source and rebuild"; return r; }
    if (bytes != sizeof(DrilEnvEvaluateDesc) || hipMemcpy(&r.desc, dptr, sizeof(r.desc), hipMemcpyDeviceToHost) != hipSuccess) {
        (void)hipGetLastError(); r.fn = r.fn_scaled = nullptr;
        r.reason = "dril_env_plugin_evaluate_desc is " + std::to_string(bytes) + " bytes, this library reads " + std::to_string(sizeof(DrilEnvEvaluateDesc)) + rebuild; return r; }
    r.has_desc = true;
    if (r.desc.abi_version != DRIL_ENV_EVALUATE_ABI) r.reason = "fused evaluation ABI " + std::to_string(r.desc.abi_version) + ", this library speaks " + std::to_string(DRIL_ENV_EVALUATE_ABI) + rebuild;
    else if (r.desc.args_size != sizeof(DrilEnvEvaluateArgs)) r.reason = "the fused evaluation's argument block is " + std::to_string(r.desc.args_size) + " bytes, this library passes " + std::to_string(sizeof(DrilEnvEvaluateArgs)) + rebuild;
    else if (r.desc.tile < 1 || r.desc.threads < r.desc.tile || r.desc.threads > 1024 || r.desc.max_width < 1) r.reason = "the fused evaluation's descriptor is out of range (tile " + std::to_string(r.desc.tile) + ", threads " + std::to_string(r.desc.threads) + ", max width " + std::to_string(r.desc.max_width) + ")";
    else if ((r.desc.has_scaled != 0) != (r.fn_scaled != nullptr)) r.reason = std::string("the fused evaluation's descriptor says has_scaled = ") + std::to_string(r.desc.has_scaled) + ", but dril_env_plugin_evaluate_scaled is " + (r.fn_scaled ? "present" : "absent");
    if (!r.reason.empty()) r.fn = r.fn_scaled = nullptr;
    return r;
}
// The declared observation space of a loaded, checked plug-in: dril_env_plugin_obs_space (one workgroup) writes low[D] | high[D] into a buffer sized from the
// descriptor.  *declared = 0 and no launch when the code object has no such kernel (built before the observation space existed, or the env declares none).
inline int read_module_obs_space(hipModule_t mod, const DrilEnvPluginDesc& d, std::vector<float>& low, std::vector<float>& high, bool* declared, std::string& msg) {
    low.assign(d.D, -INFINITY); high.assign(d.D, INFINITY); *declared = false;
    const hipFunction_t f = env_module_optional(mod, "dril_env_plugin_obs_space");
    if (!f) return DRIL_OK;
    float* buf = nullptr; std::vector<float> host(2 * (size_t)d.D);
    hipError_t e = hipMalloc((void**)&buf, host.size() * sizeof(float));
    if (e == hipSuccess) { DrilEnvPluginArgs a{}; a.E = 1; a.obs = buf; e = env_module_launch(f, a, nullptr); }
    if (e == hipSuccess) e = hipMemcpy(host.data(), buf, host.size() * sizeof(float), hipMemcpyDeviceToHost);   // (the null stream: ordered after the launch)
    if (buf) (void)hipFree(buf);
    if (e != hipSuccess) { msg = std::string("reading the plug-in's observation space (dril_env_plugin_obs_space): ") + hipGetErrorString(e); return DRIL_ERR_HIP; }
    std::copy(host.begin(), host.begin() + d.D, low.begin()); std::copy(host.begin() + d.D, host.end(), high.begin()); *declared = true;
    return DRIL_OK;
}
// dril_env_module_obs_space: load, check, read the space, unload (the checks and statuses of dril_env_module_describe)
inline int describe_module_obs_space(const char* path, int device, float* low, float* high, int32_t* declared, std::string& msg) {
    hipModule_t mod = nullptr; DrilEnvPluginDesc d{};
    int rc = load_env_module(path, device, &mod, &d, msg); if (rc) return rc;
    std::vector<float> lo, hi; bool decl = false;
    rc = read_module_obs_space(mod, d, lo, hi, &decl, msg);
    (void)hipModuleUnload(mod);
    if (rc) return rc;
    if (low) std::memcpy(low, lo.data(), lo.size() * sizeof(float));
    if (high) std::memcpy(high, hi.data(), hi.size() * sizeof(float));
    if (declared) *declared = decl ? 1 : 0;
    return DRIL_OK;
}
// ---- the envs of one handle ----
// where one act! puts its results (device arrays of E entries, terminal_obs E x D); obs: null, or where the observation AFTER the step goes (a plug-in's step kernel
// writes it in the same launch, a built-in kind's env_observe_kernel follows)
struct EnvStepOut { float* rewards; uint8_t* terminated; uint8_t* truncated; float* terminal_obs; float* obs; };

struct DeviceEnvs {
    int kind = 0, E = 0, episode_len = 0, fixed_len = 0, action_start = 0;
    uint64_t seed0 = 0;    // env e is seeded seed0 + e (reset!, and the env-keyed noise streams)
    bool ready = false;    // reset! has run
    float* state = nullptr; int32_t* step_count = nullptr; uint32_t *episode = nullptr, *gstep = nullptr; float* disc_returns = nullptr;   // E x S, E, E, E, E
    // DRIL_ENV_MODULE: the loaded plug-in (null: a built-in kind, or the host envs of DRIL_ENV_EXTERNAL); its three kernels stand in for env_reset / env_observe / env_step_kernel
    hipModule_t module = nullptr; hipFunction_t mod_reset = nullptr, mod_observe = nullptr, mod_step = nullptr; DrilEnvPluginDesc desc{};
    // the plug-in's declared observation space (obs_declared false: the env declares none; the vectors then hold -inf / +inf) and ScalingWrapperEnv
    // (scalingWrapperEnv.jl) around every env: `scaling` on = the plug-in's _scaled kernels stand where observe / step stood, agent-facing spaces Box(-1, 1)
    std::vector<float> obs_low, obs_high; bool obs_declared = false, scaling = false;
    hipFunction_t mod_observe_scaled = nullptr, mod_step_scaled = nullptr;
    EnvModuleRollout rollout;   // the plug-in's fused rollout, when its code object carries one (PPO handles: dril_rollout_fused_enable)
    EnvModuleRolloutPop rollout_pop;   // the population entry of that rollout, when the code object carries one (dril_population_join)
    uint64_t code_size = 0, code_hash = 0;   // the code object file as it was loaded: its size and the FNV-1a hash of its bytes
    EnvModuleEvaluate evaluate; // the plug-in's fused evaluation, when its code object carries one (PPO handles: path 2 of the evaluation / trajectory verbs)

    // what the envs are; for DRIL_ENV_MODULE also the plug-in: loaded, its descriptor kept, episode_len 0 replaced by the descriptor's, its three kernels found.
    // Makes `device` current when it loads; on failure nothing is held and msg says why.  no_worlds: null, or why this kind of handle takes no world (then a world is
    // refused with DRIL_ERR_UNSUPPORTED before its row count is looked at).
    int open(int kind_, int n_envs, int episode_len_, int fixed_len_, int action_start_, const char* module_path, int device, std::string& msg, const char* no_worlds = nullptr) {
        kind = kind_; E = n_envs; episode_len = episode_len_; fixed_len = fixed_len_; action_start = action_start_;
        if (kind != DRIL_ENV_MODULE) return DRIL_OK;
        const int rc = load_env_module(module_path, device, &module, &desc, msg); if (rc) return rc;
        if (desc.agents && no_worlds) { msg = std::string("env plug-in \"") + desc.name + "\" is a world of " + std::to_string(desc.agents) + " agents: " + no_worlds; release(); return DRIL_ERR_UNSUPPORTED; }
        if (desc.agents && E % desc.agents != 0) {
            msg = std::string("env plug-in \"") + desc.name + "\" is a world of " + std::to_string(desc.agents) + " agents (one row each): n_envs " + std::to_string(E) + " is not a multiple of " + std::to_string(desc.agents) + " (per rank, under data parallelism)";
            release(); return DRIL_ERR_INVALID_ARG; }
        if (episode_len == 0) episode_len = desc.episode_len;
        const char* names[3] = {"dril_env_plugin_reset", "dril_env_plugin_observe", "dril_env_plugin_step"}; hipFunction_t* fns[3] = {&mod_reset, &mod_observe, &mod_step};
        for (int i = 0; i < 3; ++i) {
            const hipError_t e = hipModuleGetFunction(fns[i], module, names[i]);
            if (e != hipSuccess) { msg = std::string("hipModuleGetFunction(") + names[i] + "): " + hipGetErrorString(e); release(); return DRIL_ERR_HIP; }
        }
        mod_observe_scaled = env_module_optional(module, "dril_env_plugin_observe_scaled"); mod_step_scaled = env_module_optional(module, "dril_env_plugin_step_scaled");
        rollout = find_module_rollout(module); rollout_pop = find_module_rollout_pop(module); evaluate = find_module_evaluate(module);
        if (!hash_code_object(module_path, &code_size, &code_hash)) { msg = std::string("cannot read code object ") + module_path; release(); return DRIL_ERR_INVALID_ARG; }
        const int rs = read_module_obs_space(module, desc, obs_low, obs_high, &obs_declared, msg);
        if (rs) release();
        return rs;
    }
    // a world (dril_env_world.h): `agents()` rows share one state of desc.S floats; a classic plug-in and a built-in kind have one agent per env.  The state array stays
    // E x S floats for either (N times what a world needs): world w lies at float offset w S, and every snapshot / restore / prefix copy of E x S (or M x S for the
    // first M rows) floats holds the worlds it has to hold
    int agents() const { return (module && desc.agents) ? desc.agents : 1; }
    bool is_world() const { return module && desc.agents != 0; }
    int n_worlds() const { return E / agents(); }
    // ScalingWrapperEnv on / off.  Legal on a plug-in handle whose envs have not been reset yet (between create and the first reset!): observations handed out
    // before would change their meaning under the caller.  Every refusal says what to do instead.
    int set_scaling(bool on, std::string& msg) {
        if (!module) { msg = "ScalingWrapperEnv by this verb wraps a device env plug-in (DRIL_ENV_MODULE): a built-in env is scaled by its own kind (DRIL_ENV_PENDULUM_SCALED, DRIL_ENV_MOUNTAINCAR_CONTINUOUS_SCALED), a host env (DRIL_ENV_EXTERNAL) on the host"; return DRIL_ERR_UNSUPPORTED; }
        if (ready) { msg = "ScalingWrapperEnv is chosen between create and the first env reset (observations already handed out would change their meaning): create a new handle"; return DRIL_ERR_INVALID_ARG; }
        if (on) {
            const std::string who = std::string("env plug-in \"") + desc.name + "\"";
            if (desc.agents) { msg = who + " is a world of " + std::to_string(desc.agents) + " agents: a world declares no observation space and carries no _scaled kernels (ScalingWrapperEnv on worlds is not built yet); scale observations and actions inside the world's own observe / step"; return DRIL_ERR_UNSUPPORTED; }
            if (desc.discrete) { msg = who + " has a Discrete action space: ScalingWrapperEnv needs Box observation and action spaces (scalingWrapperEnv.jl:22)"; return DRIL_ERR_UNSUPPORTED; }
            if (!obs_declared) { msg = who + " declares no observation space: add static constexpr float obs_low[D], obs_high[D] to the env and rebuild the code object with this library's include/device/dril_env_plugin.h"; return DRIL_ERR_UNSUPPORTED; }
            auto bad = [](float lo, float hi) { return !(std::isfinite(lo) && std::isfinite(hi) && lo < hi); };
            for (int i = 0; i < desc.D; ++i) if (bad(obs_low[i], obs_high[i])) { msg = who + ": observation dim " + std::to_string(i) + " has bounds [" + std::to_string(obs_low[i]) + ", " + std::to_string(obs_high[i]) + "]: ScalingWrapperEnv needs finite bounds with low < high in every dimension; declare such bounds (or wrap without scaling)"; return DRIL_ERR_UNSUPPORTED; }
            for (int i = 0; i < desc.A; ++i) if (bad(desc.action_low[i], desc.action_high[i])) { msg = who + ": action dim " + std::to_string(i) + " has bounds [" + std::to_string(desc.action_low[i]) + ", " + std::to_string(desc.action_high[i]) + "]: ScalingWrapperEnv needs finite bounds with low < high in every dimension"; return DRIL_ERR_UNSUPPORTED; }
            if (!mod_observe_scaled || !mod_step_scaled) { msg = who + ": the code object has no dril_env_plugin_observe_scaled / dril_env_plugin_step_scaled kernels: rebuild it with this library's include/device/dril_env_plugin.h"; return DRIL_ERR_UNSUPPORTED; }
        }
        scaling = on;
        return DRIL_OK;
    }
    // the observation space the agent sees (low[D], high[D]; either may be null): Box(-1, 1) under ScalingWrapperEnv, the declared space otherwise
    void agent_obs_space(float* low, float* high) const {
        for (int i = 0; i < desc.D; ++i) { if (low) low[i] = scaling ? -1.0f : obs_low[i]; if (high) high[i] = scaling ? 1.0f : obs_high[i]; }
    }
    // the action space the agent's adapters act on (Box plug-ins): Box(-1, 1) under ScalingWrapperEnv, the env's own bounds otherwise
    void agent_action_space(float* low, float* high) const {
        for (int i = 0; i < desc.A; ++i) { if (low) low[i] = scaling ? -1.0f : desc.action_low[i]; if (high) high[i] = scaling ? 1.0f : desc.action_high[i]; }
    }
    // the per-env arrays, on the current device; S: floats of one env's simulator state
    hipError_t alloc(int S) {
        auto dev = [](auto** p, size_t n) { return hipMalloc((void**)p, (n ? n : 1) * sizeof(**p)); };
        hipError_t e = dev(&state, (size_t)E * S);
        if (e == hipSuccess) e = dev(&step_count, (size_t)E);
        if (e == hipSuccess) e = dev(&episode, (size_t)E);
        if (e == hipSuccess) e = dev(&gstep, (size_t)E);
        if (e == hipSuccess) e = dev(&disc_returns, (size_t)E);
        return e;
    }
    void release() {
        void* ptrs[] = {state, step_count, episode, gstep, disc_returns};
        for (void* p : ptrs) if (p) (void)hipFree(p);
        state = nullptr; step_count = nullptr; episode = nullptr; gstep = nullptr; disc_returns = nullptr;
        if (module) { (void)hipModuleUnload(module); (void)hipGetLastError(); }
        module = nullptr;
    }
    // the argument block of a plug-in's three kernels: the envs; each verb adds what it reads and writes
    DrilEnvPluginArgs args() const {
        DrilEnvPluginArgs a{};
        a.E = E; a.episode_len = episode_len; a.fixed_len = fixed_len; a.action_start = action_start; a.seed0 = seed0;
        a.state = state; a.step_count = step_count; a.episode = episode; a.gstep = gstep;
        return a;
    }
    // reset!(env) / observe(env) / act!(env, actions) with auto-reset under MonitorWrapperEnv (mon all null: off), enqueued on `s`
    hipError_t reset(hipStream_t s) const {
        if (module) return env_module_launch(mod_reset, args(), s);
        return launch_env_reset(kind, E, seed0, state, step_count, episode, gstep, disc_returns, s);
    }
    hipError_t observe(float* obs, hipStream_t s) const {
        if (module) { DrilEnvPluginArgs a = args(); a.obs = obs; return env_module_launch(scaling ? mod_observe_scaled : mod_observe, a, s); }
        return launch_env_observe(kind, E, state, obs, s);
    }
    // the fused collection: ceil(E / tile) workgroups, each takes its envs through all g.T steps.  g.env: args() plus the per-step arrays and the monitor's sums
    hipError_t launch_rollout(DrilEnvRolloutArgs g, hipStream_t s) const {
        const hipFunction_t f = scaling ? rollout.fn_scaled : rollout.fn;
        if (!f) return hipErrorInvalidDeviceFunction;
        void* params[] = {&g};
        return hipModuleLaunchKernel(f, (unsigned)((E + rollout.desc.tile - 1) / rollout.desc.tile), 1, 1, (unsigned)rollout.desc.threads, 1, 1, 0, s, params, nullptr);
    }
    // n members' fused collections in one launch: grid (ceil(E / tile), n), row y takes d_members[y] (device memory; every member with this E and this code object)
    hipError_t launch_rollout_pop(const DrilEnvRolloutArgs* d_members, int n, hipStream_t s) const {
        const hipFunction_t f = scaling ? rollout_pop.fn_scaled : rollout_pop.fn;
        if (!f || n < 1) return hipErrorInvalidDeviceFunction;
        void* params[] = {&d_members, &n};
        return hipModuleLaunchKernel(f, (unsigned)((E + rollout_pop.desc.tile - 1) / rollout_pop.desc.tile), (unsigned)n, 1, (unsigned)rollout_pop.desc.threads, 1, 1, 0, s, params, nullptr);
    }
    // the fused evaluation: ceil(E / tile) workgroups, each takes its envs through the g.r.T steps of the launch
    hipError_t launch_evaluate(DrilEnvEvaluateArgs g, hipStream_t s) const {
        const hipFunction_t f = scaling ? evaluate.fn_scaled : evaluate.fn;
        if (!f) return hipErrorInvalidDeviceFunction;
        void* params[] = {&g};
        return hipModuleLaunchKernel(f, (unsigned)((E + evaluate.desc.tile - 1) / evaluate.desc.tile), 1, 1, (unsigned)evaluate.desc.threads, 1, 1, 0, s, params, nullptr);
    }
    hipError_t step(const void* actions, const EnvStepOut& o, const MonitorArgs& mon, hipStream_t s) const {
        if (module) {
            DrilEnvPluginArgs a = args();
            a.actions = actions; a.rewards = o.rewards; a.terminated = o.terminated; a.truncated = o.truncated; a.terminal_obs = o.terminal_obs; a.obs = o.obs;
            a.flags = mon.flags_out; a.mon_cur_ret = mon.cur_ret; a.mon_cur_len = mon.cur_len; a.ep_ret = mon.ep_ret; a.ep_len = mon.ep_len;
            return env_module_launch(scaling ? mod_step_scaled : mod_step, a, s);
        }
        const hipError_t e = launch_env_step(kind, E, seed0, episode_len, fixed_len, action_start, actions, state, step_count, episode, gstep,
                                             o.rewards, o.terminated, o.truncated, o.terminal_obs, mon, s);
        return (e == hipSuccess && o.obs) ? launch_env_observe(kind, E, state, o.obs, s) : e;
    }
};
}  // namespace dril
