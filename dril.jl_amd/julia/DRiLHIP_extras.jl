# DRiLHIP_extras.jl — callers either side of the path: normalisation statistics in the reference's JLD2 schema, evaluate_agent (included by DRiLHIP.jl)
# ---- normalisation statistics in the reference's JLD2 schema (normalizeWrapperEnv.jl:261-297) ----
function norm_stats(env::DeviceParallelEnv)
    D = obs_dim(env); om = Vector{Float32}(undef, D); ov = Vector{Float32}(undef, D)
    oc = Ref{Int64}(0); rm = Ref{Float32}(0); rv = Ref{Float32}(0); rc = Ref{Int64}(0)
    GC.@preserve om ov check(ccall((:dril_norm_get_stats, LIB[]), Int32,
        (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ref{Int64}, Ref{Float32}, Ref{Float32}, Ref{Int64}), handle(env), om, ov, oc, rm, rv, rc), env.handle)
    return (; obs_mean = om, obs_var = ov, obs_count = Int(oc[]), ret_mean = fill(rm[]), ret_var = fill(rv[]), ret_count = Int(rc[]))
end
function DRiL.save_normalization_stats(env::DeviceParallelEnv, filepath::String)
    s = norm_stats(env); nz = env.normalize
    return DRiL.save(filepath, Dict("obs_mean" => s.obs_mean, "obs_var" => s.obs_var, "obs_count" => s.obs_count,
        "ret_mean" => s.ret_mean, "ret_var" => s.ret_var, "ret_count" => s.ret_count,
        "clip_obs" => Float32(get(nz, :clip_obs, 10)), "clip_reward" => Float32(get(nz, :clip_reward, 10)),
        "gamma" => Float32(get(nz, :gamma, 0.99)), "epsilon" => Float32(get(nz, :epsilon, 1.0e-8))))
end
function DRiL.load_normalization_stats!(env::DeviceParallelEnv, filepath::String)
    st = DRiL.load(filepath)
    om = Float32.(st["obs_mean"]); ov = Float32.(st["obs_var"])
    GC.@preserve om ov check(ccall((:dril_norm_set_stats, LIB[]), Int32, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Int64, Float32, Float32, Int64),
        handle(env), om, ov, st["obs_count"], Float32(first(st["ret_mean"])), Float32(first(st["ret_var"])), st["ret_count"]), env.handle)
    return env
end

# ---- evaluate_agent(agent, env::DeviceParallelEnv; ...)  (src/evaluation.jl:54-143) ----
struct DrilEvalStats
    mean_reward::Float64; std_reward::Float64; mean_length::Float64; std_length::Float64
    n_episodes::Int32; n_steps::Int32
end
# dril_eval_options / dril_eval_info (include/dril_hip.h): the evaluation on the device that leaves the env side of the handle as it was (docs/evaluation.md)
struct DrilEvalOptions
    n_eval_episodes::Int32; deterministic::Int32
    seed::UInt64; has_seed::Int32
    poll_steps::Int32
    force_step_granular::Int32
    reserved::NTuple{3, Int32}
end
struct DrilEvalInfo
    path::Int32
    launches::Int32; steps_enqueued::Int32; events::Int32; reserved::NTuple{4, Int32}
end
# isolated = true: the episode accounting runs on the device and the env is left as it was — state, counters, the monitor's window, a normaliser's statistics (frozen
# for the call) — so the call may sit between two training iterations on the training env.  The default keeps the reset env and the monitor's window as before.
# persistent = true (with isolated): reserved[DRIL_EVAL_OPT_PERSISTENT = 0] — the persistent evaluate kernel wherever it can run, normalised envs included; same numbers.
function DRiL.evaluate_agent(agent, env::DeviceParallelEnv; n_eval_episodes::Int = 10, deterministic::Bool = true,
        reward_threshold::Union{Nothing, Real} = nothing, return_stats::Bool = true, warn::Bool = true, isolated::Bool = false, persistent::Bool = false, kwargs...)
    bind_agent!(env, agent, agent.algorithm); push_params!(env, agent)
    st = Ref{DrilEvalStats}(); er = Vector{Float32}(undef, n_eval_episodes); el = Vector{Int32}(undef, n_eval_episodes)
    if isolated
        o = Ref(DrilEvalOptions(Int32(n_eval_episodes), Int32(deterministic), UInt64(0), Int32(0), Int32(0), Int32(0), (Int32(persistent), Int32(0), Int32(0))))
        GC.@preserve er el check(ccall((:dril_evaluate_agent_device, LIB[]), Int32, (Ptr{Cvoid}, Ref{DrilEvalOptions}, Ref{DrilEvalStats}, Ptr{Float32}, Ptr{Int32}, Ptr{DrilEvalInfo}),
            env.handle, o, st, er, el, C_NULL), env.handle)
    else
        GC.@preserve er el check(ccall((:dril_evaluate_agent, LIB[]), Int32, (Ptr{Cvoid}, Int32, Int32, Ref{DrilEvalStats}, Ptr{Float32}, Ptr{Int32}),
            env.handle, n_eval_episodes, deterministic, st, er, el), env.handle)
    end
    s = st[]
    if reward_threshold !== nothing && s.mean_reward < reward_threshold
        error("Mean reward below threshold: $(round(s.mean_reward, digits = 2)) < $(reward_threshold)")            # evaluation.jl:131-135
    end
    return return_stats ? (; mean_reward = s.mean_reward, std_reward = s.std_reward, mean_length = s.mean_length, std_length = s.std_length) :
        (er, Int.(el))
end


# ---- collect_trajectory(agent, env::DeviceParallelEnv; ...)  (src/utils/trajectory_utils.jl:3-49) ----
# dril_traj_options / dril_traj_info (include/dril_hip.h): the reference loop on the device, once per recorded env, leaving the env as it was (docs/evaluation.md)
struct DrilTrajOptions
    n_trajectories::Int32; max_steps::Int32; deterministic::Int32
    has_seed::Int32; seed::UInt64
    poll_steps::Int32; final_original::Int32
    reserved::NTuple{5, Int32}
end
struct DrilTrajInfo
    capacity::Int32; steps_enqueued::Int32; launches::Int32; longest::Int32; cut_by_max_steps::Int32; reserved::NTuple{3, Int32}
end
# -> (observations, actions, rewards) as the reference returns them (L + 1 original observations, L env actions, L raw rewards); n_trajectories > 1: a vector of such
# tuples, envs 1..n of the parallel env, each its first episode after the reset.  A NormalizeWrapperEnv around the device env is a mode of its handle: applied frozen.
# persistent = true: reserved[DRIL_TRAJ_OPT_PERSISTENT = 0] — the recording inside the persistent evaluate kernel where it can run (silent fall-back elsewhere); same recording.
function DRiL.collect_trajectory(agent, env::DeviceParallelEnv; max_steps::Union{Int, Nothing} = nothing, deterministic::Bool = true, n_trajectories::Int = 1, persistent::Bool = false, kwargs...)
    bind_agent!(env, agent, agent.algorithm); push_params!(env, agent)
    h = env.handle
    o = Ref(DrilTrajOptions(Int32(n_trajectories), Int32(max_steps === nothing ? 0 : max_steps), Int32(deterministic), Int32(0), UInt64(0), Int32(0), Int32(0),
        (Int32(persistent), Int32(0), Int32(0), Int32(0), Int32(0))))
    cap = Ref{Int32}(0)
    check(ccall((:dril_trajectory_capacity, LIB[]), Int32, (Ptr{Cvoid}, Ref{DrilTrajOptions}, Ref{Int32}), h, o, cap), h)
    D = obs_dim(env); T = Int(cap[]); M = n_trajectories; disc = is_discrete(env)
    A = disc ? 1 : Int(ccall((:dril_action_dim, LIB[]), Int32, (Ptr{Cvoid},), h))
    obs = Array{Float32}(undef, D, T + 1, M); rew = Matrix{Float32}(undef, T, M); len = Vector{Int32}(undef, M); flags = Vector{UInt8}(undef, M)
    act = disc ? Array{Int32}(undef, 1, T, M) : Array{Float32}(undef, A, T, M)
    GC.@preserve obs act rew len flags check(ccall((:dril_collect_trajectory_device, LIB[]), Int32, (Ptr{Cvoid}, Ref{DrilTrajOptions}, Ptr{Float32}, Ptr{Cvoid}, Ptr{Float32}, Ptr{Int32}, Ptr{UInt8}, Ptr{DrilTrajInfo}),
        h, o, obs, act, rew, len, flags, C_NULL), h)
    any(f -> f & 0x04 != 0, flags) && @warn "Max steps reached"                                                    # trajectory_utils.jl:39
    trajs = map(1:M) do m
        L = Int(len[m])
        ([obs[:, t, m] for t in 1:(L + 1)], disc ? [Int(act[1, t, m]) for t in 1:L] : [act[:, t, m] for t in 1:L], [rew[t, m] for t in 1:L])
    end
    return M == 1 ? trajs[1] : trajs
end


# ---- deployment policies on the device (include/dril_policy.h): the device twin of extract_policy (src/deployment/deployment_policy.jl) ----
# DRiL.extract_policy(agent[, norm_env]) keeps working on the host parameters train! writes back; a DevicePolicy is the same thing as one light device object
# (actor + adapter + frozen observation statistics) that answers in one kernel launch.  Calls on one DevicePolicy must not overlap.
mutable struct DevicePolicy
    ptr::Ptr{Cvoid}
    obs_dim::Int
    action_dim::Int
    discrete::Bool
end
policy_last_error(p) = unsafe_string(ccall((:dril_policy_last_error, LIB[]), Cstring, (Ptr{Cvoid},), p))
policy_check(rc::Int32, p = C_NULL) = rc == 0 ? nothing : error("libdril_hip (policy) status $rc: $(policy_last_error(p))")
function destroy!(p::DevicePolicy)
    p.ptr == C_NULL || ccall((:dril_policy_destroy, LIB[]), Int32, (Ptr{Cvoid},), p.ptr)
    p.ptr = C_NULL
    return nothing
end
function wrap_policy(ptr::Ptr{Cvoid}, obs_dim, action_dim, discrete)
    p = DevicePolicy(ptr, Int(obs_dim), Int(action_dim), discrete)
    finalizer(destroy!, p)
    return p
end
"`extract_device_policy(agent, env::DeviceParallelEnv; with_norm)`: extract_policy(agent) / extract_policy(agent, norm_env) as a device-to-device snapshot of the env's PPO handle; with_norm defaults to whether the env carries NormalizeWrapperEnv keywords"
function extract_device_policy(agent, env::DeviceParallelEnv; with_norm::Bool = env.normalize !== nothing)
    bind_agent!(env, agent, agent.algorithm); push_params!(env, agent)
    h = env.handle; pp = Ref{Ptr{Cvoid}}(C_NULL)
    policy_check(ccall((:dril_policy_from_handle, LIB[]), Int32, (Ptr{Cvoid}, Int32, Ref{Ptr{Cvoid}}), h, Int32(with_norm), pp))
    return wrap_policy(pp[], ccall((:dril_obs_dim, LIB[]), Int32, (Ptr{Cvoid},), h), ccall((:dril_action_dim, LIB[]), Int32, (Ptr{Cvoid},), h),
        ccall((:dril_is_discrete, LIB[]), Int32, (Ptr{Cvoid},), h) != 0)
end
"`extract_device_policy_sac(h; with_norm)`: the same from a live SAC handle (a `Ptr{Cvoid}` of dril_sac_create), e.g. inside a callback of train!(agent, env, alg::SAC, ...)"
function extract_device_policy_sac(h::Ptr{Cvoid}; with_norm::Bool = false)
    pp = Ref{Ptr{Cvoid}}(C_NULL)
    policy_check(ccall((:dril_policy_from_sac_handle, LIB[]), Int32, (Ptr{Cvoid}, Int32, Ref{Ptr{Cvoid}}), h, Int32(with_norm), pp))
    return wrap_policy(pp[], ccall((:dril_sac_obs_dim, LIB[]), Int32, (Ptr{Cvoid},), h), ccall((:dril_sac_action_dim, LIB[]), Int32, (Ptr{Cvoid},), h), false)
end
# policy(obs; deterministic, seed): one observation (a vector) -> one env action; a vector of observations -> a vector of env actions (deployment_policy.jl:25-41).
# Sampling draws from the policy's own Philox stream; `seed` restarts it
function (p::DevicePolicy)(obs; deterministic::Bool = true, seed::Union{Nothing, Integer} = nothing)
    single = obs isa AbstractVector{<:Real}
    cols = single ? [obs] : obs
    B = length(cols)
    x = Matrix{Float32}(undef, p.obs_dim, B)
    for (j, o) in enumerate(cols)
        x[:, j] .= vec(o)
    end
    seed === nothing || policy_check(ccall((:dril_policy_set_seed, LIB[]), Int32, (Ptr{Cvoid}, UInt64), p.ptr, UInt64(seed)), p.ptr)
    if p.discrete
        a = Vector{Int32}(undef, B)
        GC.@preserve x a policy_check(ccall((:dril_policy_act, LIB[]), Int32, (Ptr{Cvoid}, Ptr{Float32}, Int64, Int32, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
            p.ptr, x, B, Int32(deterministic), C_NULL, C_NULL, a), p.ptr)
        acts = Int.(a)
        return single ? acts[1] : acts
    end
    a = Matrix{Float32}(undef, p.action_dim, B)
    GC.@preserve x a policy_check(ccall((:dril_policy_act, LIB[]), Int32, (Ptr{Cvoid}, Ptr{Float32}, Int64, Int32, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
        p.ptr, x, B, Int32(deterministic), C_NULL, C_NULL, a), p.ptr)
    acts = [a[:, j] for j in 1:B]
    return single ? acts[1] : acts
end


# =====================================================================================================================
# SAC: train!(agent, env::DeviceParallelEnv, alg::SAC, max_steps)  (src/algorithms/sac.jl:406-549) over include/dril_sac.h
