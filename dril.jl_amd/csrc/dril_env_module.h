// dril_env_module.h — loading a device env plug-in (include/device/dril_env_plugin.h): the ONE definition of the path checks, the descriptor checks and the load order
// that dril_create_with_env_module / dril_env_module_describe (dril_api.hip) and dril_sac_create_with_env_module (dril_sac.hip) share, plus the launch of a plug-in kernel.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <string>

#include "../../include/dril_hip.h"
#include "../../include/device/dril_env_plugin.h"   // DrilEnvPluginDesc / DrilEnvPluginArgs: the same definitions a plug-in is compiled with

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
}  // namespace dril
