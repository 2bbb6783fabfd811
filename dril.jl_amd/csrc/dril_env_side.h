// dril_env_side.h — the env side of a handle: the envs a PPO handle (dril_api.hip) or a SAC handle (dril_sac.hip) steps on the device, whichever they are — a built-in
// kind (dril_env_kinds.h; the env kernels of dril_kernels.hip) or a device env plug-in (include/device/dril_env_plugin.h; a HIP module loaded at create).  The ONE
// definition of loading a plug-in (path checks, descriptor checks, load order), of the argument block its kernels take, and of reset! / observe / act! over either.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <string>

#include "../../include/dril_hip.h"
#include "../../include/device/dril_env_plugin.h"   // DrilEnvPluginDesc / DrilEnvPluginArgs: the same definitions a plug-in is compiled with
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
    if (d.S < 1 || d.S > DRIL_ENV_PLUGIN_MAX_S || d.D < 1 || d.D > DRIL_ENV_PLUGIN_MAX_D || d.A < 1 || d.A > DRIL_ENV_PLUGIN_MAX_A || d.episode_len < 1) {
        msg = "env plug-in descriptor out of range: S " + std::to_string(d.S) + " (1..64), D " + std::to_string(d.D) + " (1..1024), A " + std::to_string(d.A) + " (1..64), episode_len " + std::to_string(d.episode_len) + " (>= 1)"; return DRIL_ERR_UNSUPPORTED; }
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

    // what the envs are; for DRIL_ENV_MODULE also the plug-in: loaded, its descriptor kept, episode_len 0 replaced by the descriptor's, its three kernels found.
    // Makes `device` current when it loads; on failure nothing is held and msg says why.
    int open(int kind_, int n_envs, int episode_len_, int fixed_len_, int action_start_, const char* module_path, int device, std::string& msg) {
        kind = kind_; E = n_envs; episode_len = episode_len_; fixed_len = fixed_len_; action_start = action_start_;
        if (kind != DRIL_ENV_MODULE) return DRIL_OK;
        const int rc = load_env_module(module_path, device, &module, &desc, msg); if (rc) return rc;
        if (episode_len == 0) episode_len = desc.episode_len;
        const char* names[3] = {"dril_env_plugin_reset", "dril_env_plugin_observe", "dril_env_plugin_step"}; hipFunction_t* fns[3] = {&mod_reset, &mod_observe, &mod_step};
        for (int i = 0; i < 3; ++i) {
            const hipError_t e = hipModuleGetFunction(fns[i], module, names[i]);
            if (e != hipSuccess) { msg = std::string("hipModuleGetFunction(") + names[i] + "): " + hipGetErrorString(e); release(); return DRIL_ERR_HIP; }
        }
        return DRIL_OK;
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
        if (module) { DrilEnvPluginArgs a = args(); a.obs = obs; return env_module_launch(mod_observe, a, s); }
        return launch_env_observe(kind, E, state, obs, s);
    }
    hipError_t step(const void* actions, const EnvStepOut& o, const MonitorArgs& mon, hipStream_t s) const {
        if (module) {
            DrilEnvPluginArgs a = args();
            a.actions = actions; a.rewards = o.rewards; a.terminated = o.terminated; a.truncated = o.truncated; a.terminal_obs = o.terminal_obs; a.obs = o.obs;
            a.flags = mon.flags_out; a.mon_cur_ret = mon.cur_ret; a.mon_cur_len = mon.cur_len; a.ep_ret = mon.ep_ret; a.ep_len = mon.ep_len;
            return env_module_launch(mod_step, a, s);
        }
        const hipError_t e = launch_env_step(kind, E, seed0, episode_len, fixed_len, action_start, actions, state, step_count, episode, gstep,
                                             o.rewards, o.terminated, o.truncated, o.terminal_obs, mon, s);
        return (e == hipSuccess && o.obs) ? launch_env_observe(kind, E, state, o.obs, s) : e;
    }
};
}  // namespace dril
