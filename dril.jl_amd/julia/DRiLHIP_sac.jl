# DRiLHIP_sac.jl — the off-policy path: train!(agent, env, alg::SAC, ...) over include/dril_sac.h (included by DRiLHIP.jl)
# =====================================================================================================================
# struct dril_sac_config / dril_sac_stats (include/dril_sac.h) — isbits, C layout
struct DrilSacConfig
    abi_version::UInt32; env_kind::Int32; n_envs::Int32; episode_len::Int32
    hidden1::Int32; hidden2::Int32; activation::Int32
    buffer_capacity::Int64; start_steps::Int32; batch_size::Int32
    tau::Float32; gamma::Float32
    train_freq::Int32; gradient_steps::Int32; target_update_interval::Int32
    auto_ent_coef::Int32; ent_coef_init::Float32; auto_target_entropy::Int32; target_entropy::Float32
    learning_rate::Float32; adam_beta1::Float32; adam_beta2::Float32; adam_eps::Float32
    seed::UInt64; device::Int32; profile_events::Int32
    ext_obs_dim::Int32; ext_action_dim::Int32; ext_action_low::Float32; ext_action_high::Float32
    reserved::NTuple{4, Int32}
end
struct DrilSacStats
    actor_loss::Float32; critic_loss::Float32; entropy_loss::Float32; mean_q_values::Float32; entropy_coefficient::Float32; grad_norm::Float32
    has_entropy_loss::Int32; reserved::Int32
end
sac_check(rc::Int32, h = C_NULL) = rc == 0 ? nothing :
    error("libdril_hip (SAC) status $rc: " * unsafe_string(ccall((:dril_sac_last_error, LIB[]), Cstring, (Ptr{Cvoid},), h)))

# ContinuousActorCriticLayer{QCritic}: actor_head = Chain(mlp, ReshapeLayer), critic_head = Parallel(vcat, mlp, mlp) (layer_helpers.jl:77,100-112)
function sac_flatten_params(ps)
    parts = Vector{Float32}[]
    for head in (mlp_of(ps.actor_head), ps.critic_head.layer_1, ps.critic_head.layer_2), l in (:layer_1, :layer_2, :layer_3)
        push!(parts, vec(getproperty(head, l).weight)); push!(parts, vec(getproperty(head, l).bias))
    end
    push!(parts, vec(ps.log_std))
    return reduce(vcat, parts)
end
function sac_scatter_params!(ps, flat::Vector{Float32})
    off = 0
    for head in (mlp_of(ps.actor_head), ps.critic_head.layer_1, ps.critic_head.layer_2), l in (:layer_1, :layer_2, :layer_3)
        for arr in (getproperty(head, l).weight, getproperty(head, l).bias)
            n = length(arr); copyto!(arr, 1, flat, off + 1, n); off += n
        end
    end
    copyto!(ps.log_std, 1, flat, off + 1, length(ps.log_std))
    return ps
end
function sac_flatten_targets(tp)
    parts = Vector{Float32}[]
    for head in (tp.critic_head.layer_1, tp.critic_head.layer_2), l in (:layer_1, :layer_2, :layer_3)
        push!(parts, vec(getproperty(head, l).weight)); push!(parts, vec(getproperty(head, l).bias))
    end
    return reduce(vcat, parts)
end
function sac_scatter_targets!(tp, flat::Vector{Float32})
    off = 0
    for head in (tp.critic_head.layer_1, tp.critic_head.layer_2), l in (:layer_1, :layer_2, :layer_3)
        for arr in (getproperty(head, l).weight, getproperty(head, l).bias)
            n = length(arr); copyto!(arr, 1, flat, off + 1, n); off += n
        end
    end
    return tp
end

# dril_sac_env_module_info_of: spaces and bounds of the plug-in behind a live SAC handle (the byte layout describe_env_module reads)
function sac_env_module_info(h::Ptr{Cvoid})
    buf = zeros(UInt8, MODULE_INFO_BYTES)
    sac_check(ccall((:dril_sac_env_module_info_of, LIB[]), Int32, (Ptr{Cvoid}, Ptr{Cvoid}), h, buf), h)
    i32 = reinterpret(Int32, buf[5:24]); A = Int(i32[3])
    return (state_dim = Int(i32[1]), obs_dim = Int(i32[2]), action_dim = A, discrete = i32[4] != 0, episode_len = Int(i32[5]),
        low = collect(reinterpret(Float32, buf[25:280]))[1:A], high = collect(reinterpret(Float32, buf[281:536]))[1:A])
end

function sac_config(env::DeviceParallelEnv, alg::DRiL.SAC, agent)
    is_discrete(env) && error("SAC needs a Box action space (sac.jl:74): DeviceParallelEnv(:Pendulum | :ScaledPendulum | :MountainCarContinuous | :ScaledMountainCarContinuous, ...) or OnDeviceModule over a Box plug-in")
    hd = hidden_dims_of(agent.train_state.parameters)
    act = agent.layer.actor_head.layers[1].layers[1].activation === DRiL.Lux.relu ? Int32(1) : Int32(0)   # SACLayer default relu (sac.jl:77)
    ec = alg.ent_coef
    auto = ec isa DRiL.AutoEntropyCoefficient
    auto_t = auto && ec.target isa DRiL.AutoEntropyTarget
    return DrilSacConfig(UInt32(1), ENV_KINDS[env.kind], env.n_envs, env.max_steps, hd[1], hd[2], act,
        alg.buffer_capacity, alg.start_steps, alg.batch_size, alg.tau, alg.gamma, alg.train_freq, alg.gradient_steps, alg.target_update_interval,
        Int32(auto), auto ? Float32(ec.initial_value) : Float32(ec.coef), Int32(auto ? auto_t : true),
        auto && !auto_t ? Float32(ec.target.target) : 0.0f0,
        alg.learning_rate, 0.9f0, 0.999f0, 1.0f-8,                                                # Optimisers.Adam(lr) defaults, agent_methods.jl:116-118
        env.seed, env.device, Int32(0), 0, 0, 0.0f0, 0.0f0, ntuple(_ -> Int32(0), 4))
end

# struct dril_sac_normalize_config (include/dril_sac.h): the keywords of NormalizeWrapperEnv (normalizeWrapperEnv.jl:71-80)
struct DrilSacNormalizeConfig
    training::Int32; norm_obs::Int32; norm_reward::Int32
    clip_obs::Float32; clip_reward::Float32
    gamma::Float32; epsilon::Float32
    reserved::Int32
end
# NormalizeWrapperEnv around the handle's device envs from the env's `normalize` keywords (a NamedTuple; missing keys take the reference's defaults); `training`
# overrides the keyword (evaluate_agent: set_training(eval_env, false))
function sac_normalize_enable!(h::Ptr{Cvoid}, nz::NamedTuple; training::Union{Nothing, Bool} = nothing)
    g(k, d) = get(nz, k, d)
    cfg = Ref(DrilSacNormalizeConfig(Int32(something(training, g(:training, true))), Int32(g(:norm_obs, true)), Int32(g(:norm_reward, true)),
        Float32(g(:clip_obs, 10.0f0)), Float32(g(:clip_reward, 10.0f0)), Float32(g(:gamma, 0.99f0)), Float32(g(:epsilon, 1.0f-8)), Int32(0)))
    sac_check(ccall((:dril_sac_normalize_enable, LIB[]), Int32, (Ptr{Cvoid}, Ref{DrilSacNormalizeConfig}), h, cfg), h)
    return h
end
sac_normalize_set_training!(h::Ptr{Cvoid}, training::Bool) =
    (sac_check(ccall((:dril_sac_normalize_set_training, LIB[]), Int32, (Ptr{Cvoid}, Int32), h, Int32(training)), h); h)
# obs_rms / ret_rms of the wrapper behind a SAC handle: the fields of save_normalization_stats (normalizeWrapperEnv.jl:261-277)
function sac_norm_stats(h::Ptr{Cvoid})
    D = Int(ccall((:dril_sac_obs_dim, LIB[]), Int32, (Ptr{Cvoid},), h))
    om = Vector{Float32}(undef, D); ov = Vector{Float32}(undef, D); oc = Ref{Int64}(0); rc = Ref{Int64}(0); rm = Ref{Float32}(0); rv = Ref{Float32}(0)
    GC.@preserve om ov sac_check(ccall((:dril_sac_normalize_get_stats, LIB[]), Int32,
        (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ref{Int64}, Ref{Float32}, Ref{Float32}, Ref{Int64}), h, om, ov, oc, rm, rv, rc), h)
    return (obs_mean = om, obs_var = ov, obs_count = oc[], ret_mean = rm[], ret_var = rv[], ret_count = rc[])
end
# load_normalization_stats! / sync_normalization_stats! (:280-309) into the wrapper behind a SAC handle
function sac_set_norm_stats!(h::Ptr{Cvoid}, s)
    om = Vector{Float32}(vec(s.obs_mean)); ov = Vector{Float32}(vec(s.obs_var))
    GC.@preserve om ov sac_check(ccall((:dril_sac_normalize_set_stats, LIB[]), Int32, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Int64, Float32, Float32, Int64),
        h, om, ov, Int64(s.obs_count), Float32(first(s.ret_mean)), Float32(first(s.ret_var)), Int64(s.ret_count)), h)
    return h
end
# get_original_obs / get_original_rewards (:225-226): (D x n_envs matrix, n_envs vector)
function sac_norm_original(h::Ptr{Cvoid}, n_envs::Int)
    D = Int(ccall((:dril_sac_obs_dim, LIB[]), Int32, (Ptr{Cvoid},), h))
    obs = Matrix{Float32}(undef, D, n_envs); rew = Vector{Float32}(undef, n_envs)
    GC.@preserve obs rew sac_check(ccall((:dril_sac_normalize_get_original, LIB[]), Int32, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}), h, obs, rew), h)
    return obs, rew
end

# a SAC handle over a device env: built-in kind or the caller's code object; MonitorWrapperEnv switched on when the env carries a window, NormalizeWrapperEnv when it
# carries `normalize` keywords (built-in kinds and OnDeviceModule alike: the SAC handle's wrapper takes any observation width)
function sac_create(env::DeviceParallelEnv, alg::DRiL.SAC, agent)
    cfg = Ref(sac_config(env, alg, agent)); hp = Ref{Ptr{Cvoid}}(C_NULL)
    if env.kind === :Module      # OnDeviceModule: the env is the caller's code object; spaces and per-dimension Box bounds are its descriptor's
        sac_check(ccall((:dril_sac_create_with_env_module, LIB[]), Int32, (Ref{DrilSacConfig}, Cstring, Ref{Ptr{Cvoid}}), cfg, MODULE_ENVS[env].path, hp))
    else
        sac_check(ccall((:dril_sac_create, LIB[]), Int32, (Ref{DrilSacConfig}, Ref{Ptr{Cvoid}}), cfg, hp))
    end
    h = hp[]
    if env.kind === :Module && MODULE_ENVS[env].scaling      # ScalingWrapperEnv: before the first reset, inside NormalizeWrapperEnv; the adapters then see Box(-1, 1)
        rc = ccall((:dril_sac_scaling_enable, LIB[]), Int32, (Ptr{Cvoid}, Int32), h, Int32(1))
        rc == 0 || (msg = unsafe_string(ccall((:dril_sac_last_error, LIB[]), Cstring, (Ptr{Cvoid},), h)); ccall((:dril_sac_destroy, LIB[]), Int32, (Ptr{Cvoid},), h); error("libdril_hip (SAC) status $rc: " * msg))
    end
    if env.monitor_window > 0
        rc = ccall((:dril_sac_monitor_enable, LIB[]), Int32, (Ptr{Cvoid}, Int32), h, env.monitor_window)
        rc == 0 || (msg = unsafe_string(ccall((:dril_sac_last_error, LIB[]), Cstring, (Ptr{Cvoid},), h)); ccall((:dril_sac_destroy, LIB[]), Int32, (Ptr{Cvoid},), h); error("libdril_hip (SAC) status $rc: " * msg))
    end
    if env.normalize !== nothing
        try
            sac_normalize_enable!(h, env.normalize)
        catch
            ccall((:dril_sac_destroy, LIB[]), Int32, (Ptr{Cvoid},), h)
            rethrow()
        end
    end
    return h
end
# log_stats(env::MonitorWrapperEnv, logger) (monitorWrapperEnv.jl:64-70, called by sac.jl:307) from the SAC handle's window of finished episodes
function sac_log_stats(h::Ptr{Cvoid}, env::DeviceParallelEnv, logger)
    env.monitor_window > 0 || return nothing
    r = Ref{Float32}(0); l = Ref{Float32}(0); n = Ref{Int32}(0)
    sac_check(ccall((:dril_sac_monitor_get_stats, LIB[]), Int32, (Ptr{Cvoid}, Ref{Float32}, Ref{Float32}, Ref{Int32}), h, r, l, n), h)
    if n[] > 0
        DRiL.log_scalar!(logger, "env/ep_rew_mean", r[]); DRiL.log_scalar!(logger, "env/ep_len_mean", l[])
    end
    return (ep_rew_mean = r[], ep_len_mean = l[], n_episodes = Int(n[]))
end
function sac_push_agent!(h::Ptr{Cvoid}, agent)
    flat = sac_flatten_params(agent.train_state.parameters); tgt = sac_flatten_targets(agent.aux.Q_target_parameters)
    GC.@preserve flat tgt begin
        sac_check(ccall((:dril_sac_set_params, LIB[]), Int32, (Ptr{Cvoid}, Ptr{Float32}, Csize_t), h, flat, length(flat)), h)
        sac_check(ccall((:dril_sac_set_target_params, LIB[]), Int32, (Ptr{Cvoid}, Ptr{Float32}, Csize_t), h, tgt, length(tgt)), h)
    end
    sac_check(ccall((:dril_sac_set_log_ent_coef, LIB[]), Int32, (Ptr{Cvoid}, Float32), h, first(agent.aux.ent_train_state.parameters.log_ent_coef)), h)
    return flat, tgt
end

"""
    evaluate_agent(agent::SACAgent, env::DeviceParallelEnv; n_eval_episodes = 10, deterministic = true, ...)

`evaluate_agent` (src/evaluation.jl:54-143) of a SAC agent on a device env (built-in Box kind or `OnDeviceModule`): the agent's actor steps `n_envs` envs
seeded `env.seed + i` on the device, the episode accounting stays there (dril_sac_evaluate_agent).  Same keywords and return shapes as the reference.
An env with `normalize` keywords is evaluated under NormalizeWrapperEnv with training off; `normalize_stats` (what `sac_norm_stats` returned for the training handle)
are the statistics it normalises with.  Episode returns are raw.
"""
function DRiL.evaluate_agent(agent::SACAgent, env::DeviceParallelEnv; n_eval_episodes::Int = 10, deterministic::Bool = true,
        reward_threshold::Union{Nothing, Real} = nothing, return_stats::Bool = true, warn::Bool = true, normalize_stats = nothing, kwargs...)
    h = sac_create(env, agent.algorithm, agent)
    try
        sac_push_agent!(h, agent)
        if env.normalize !== nothing      # the reference's arrangement (normalizeWrapperEnv.jl:245-249,299-309): the training statistics (sac_norm_stats of the training handle), frozen
            sac_normalize_set_training!(h, false)
            normalize_stats === nothing || sac_set_norm_stats!(h, normalize_stats)
        end
        st = Ref{DrilEvalStats}(); er = Vector{Float32}(undef, n_eval_episodes); el = Vector{Int32}(undef, n_eval_episodes)
        GC.@preserve er el sac_check(ccall((:dril_sac_evaluate_agent, LIB[]), Int32, (Ptr{Cvoid}, Int32, Int32, UInt64, Ref{DrilEvalStats}, Ptr{Float32}, Ptr{Int32}),
            h, n_eval_episodes, deterministic, env.seed, st, er, el), h)
        s = st[]
        if reward_threshold !== nothing && s.mean_reward < reward_threshold
            error("Mean reward below threshold: $(round(s.mean_reward, digits = 2)) < $(reward_threshold)")            # evaluation.jl:131-135
        end
        return return_stats ? (; mean_reward = s.mean_reward, std_reward = s.std_reward, mean_length = s.mean_length, std_length = s.std_length) :
            (er, Int.(el))
    finally
        ccall((:dril_sac_destroy, LIB[]), Int32, (Ptr{Cvoid},), h)
    end
end

"""
    collect_trajectory(agent::SACAgent, env::DeviceParallelEnv; max_steps = nothing, deterministic = true, n_trajectories = 1, ...)

`collect_trajectory` (src/utils/trajectory_utils.jl:3-49) of a SAC agent on a device env (built-in Box kind or `OnDeviceModule`), on a throw-away handle built as
`evaluate_agent` builds its own (dril_sac_collect_trajectory): `(observations, actions, rewards)` as the reference returns them (L + 1 original observations, L env
actions, L raw rewards); `n_trajectories > 1`: a vector of such tuples, envs 1..n of the parallel env, each its first episode after the reset.  An env with
`normalize` keywords runs under NormalizeWrapperEnv with training off and `normalize_stats`; the recording is raw.
"""
function DRiL.collect_trajectory(agent::SACAgent, env::DeviceParallelEnv; max_steps::Union{Int, Nothing} = nothing, deterministic::Bool = true, n_trajectories::Int = 1,
        normalize_stats = nothing, kwargs...)
    h = sac_create(env, agent.algorithm, agent)
    try
        sac_push_agent!(h, agent)
        if env.normalize !== nothing
            sac_normalize_set_training!(h, false)
            normalize_stats === nothing || sac_set_norm_stats!(h, normalize_stats)
        end
        o = Ref(DrilTrajOptions(Int32(n_trajectories), Int32(max_steps === nothing ? 0 : max_steps), Int32(deterministic), Int32(1), UInt64(env.seed), Int32(0), Int32(0),
            (Int32(0), Int32(0), Int32(0), Int32(0), Int32(0))))
        cap = Ref{Int32}(0)
        sac_check(ccall((:dril_sac_trajectory_capacity, LIB[]), Int32, (Ptr{Cvoid}, Ref{DrilTrajOptions}, Ref{Int32}), h, o, cap), h)
        D = Int(ccall((:dril_sac_obs_dim, LIB[]), Int32, (Ptr{Cvoid},), h)); A = Int(ccall((:dril_sac_action_dim, LIB[]), Int32, (Ptr{Cvoid},), h))
        T = Int(cap[]); M = n_trajectories
        obs = Array{Float32}(undef, D, T + 1, M); act = Array{Float32}(undef, A, T, M); rew = Matrix{Float32}(undef, T, M)
        len = Vector{Int32}(undef, M); flags = Vector{UInt8}(undef, M)
        GC.@preserve obs act rew len flags sac_check(ccall((:dril_sac_collect_trajectory, LIB[]), Int32,
            (Ptr{Cvoid}, Ref{DrilTrajOptions}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Int32}, Ptr{UInt8}, Ptr{DrilTrajInfo}),
            h, o, obs, act, rew, len, flags, C_NULL), h)
        any(f -> f & 0x04 != 0, flags) && @warn "Max steps reached"                                                # trajectory_utils.jl:39
        trajs = map(1:M) do m
            L = Int(len[m])
            ([obs[:, t, m] for t in 1:(L + 1)], [act[:, t, m] for t in 1:L], [rew[t, m] for t in 1:L])
        end
        return M == 1 ? trajs[1] : trajs
    finally
        ccall((:dril_sac_destroy, LIB[]), Int32, (Ptr{Cvoid},), h)
    end
end

"""
    train!(agent, env::DeviceParallelEnv, alg::SAC, max_steps) -> (agent, nothing, training_stats, to)

Same contract as `train!(agent, replay_buffer, env, alg::SAC, max_steps)` (sac.jl:414-549) with the ReplayBuffer resident on the device
(second return value `nothing`; read it through `dril_sac_replay_copy_out`).  Callbacks with `on_step` hooks are not supported on this path.
An env built with `normalize = (; ...)` trains under NormalizeWrapperEnv on the device (dril_sac_normalize_enable: any observation width, plug-ins included);
`normalization_stats = Ref{Any}()` receives the final statistics (`sac_norm_stats`), which `evaluate_agent(...; normalize_stats = ...)` takes.
"""
function train!(agent::SACAgent, env::DeviceParallelEnv, alg::DRiL.SAC, max_steps::Int; ad_type = nothing, callbacks = nothing,
        normalization_stats::Union{Nothing, Base.RefValue} = nothing)
    T = typeof(alg.learning_rate)
    if has_step_hooks(callbacks)      # on_step hooks: the reference's own train! over this env's step-granular verbs
        kw = isnothing(ad_type) ? (; callbacks = callbacks) : (; ad_type = ad_type, callbacks = callbacks)
        return invoke(train!, Tuple{SACAgent, AbstractParallelEnv, DRiL.SAC, Int}, agent, env, alg, max_steps; kw...)
    end
    to = TimerOutput()
    h = sac_create(env, alg, agent)      # (env.monitor_window > 0: MonitorWrapperEnv on, its statistics logged below)
    try
        if env.kind === :Module      # the file may have changed since OnDeviceModule described it: the layer was built from that description
            info = sac_env_module_info(h)
            (info.obs_dim, info.action_dim) == (obs_dim(env), length(action_space(env).low)) || error("the plug-in behind the SAC handle is not the one OnDeviceModule described")
        end
        flat, tgt = sac_push_agent!(h, agent)
        sac_check(ccall((:dril_sac_env_reset, LIB[]), Int32, (Ptr{Cvoid}, UInt64), h, env.seed), h)
        n_envs = env.n_envs                                                                       # schedule: sac.jl:436-447
        total_start = alg.start_steps > 0 ? alg.start_steps : alg.train_freq * n_envs
        adjusted = max(1, div(total_start, n_envs)) * n_envs
        iterations = div(max_steps - adjusted, alg.train_freq * n_envs) + 1
        n_upd = DRiL.get_gradient_steps(alg, alg.train_freq, n_envs)
        cap = max(1, iterations * n_upd)
        st = Vector{DrilSacStats}(undef, cap); fps = Vector{Float64}(undef, max(1, iterations))
        nu = Ref{Int64}(0); it = Ref{Int32}(0); tot = Ref{Int64}(0)
        !isnothing(callbacks) && !all(c -> DRiL.on_training_start(c, Dict{Symbol, Any}(:agent => agent, :env => env, :alg => alg)), callbacks) && return agent, nothing, DRiL.SACTrainingStats{T}()
        @timeit to "training_loop" GC.@preserve st fps sac_check(ccall((:dril_sac_train, LIB[]), Int32,
            (Ptr{Cvoid}, Int64, Ptr{DrilSacStats}, Int64, Ref{Int64}, Ptr{Float64}, Int64, Ref{Int32}, Ref{Int64}),
            h, max_steps, st, cap, nu, fps, length(fps), it, tot), h)
        ts = DRiL.SACTrainingStats{T}()                                                            # sac.jl:243-257
        for k in 1:min(nu[], cap)
            s = st[k]
            push!(ts.actor_losses, s.actor_loss); push!(ts.critic_losses, s.critic_loss); s.has_entropy_loss != 0 && push!(ts.entropy_losses, s.entropy_loss)
            push!(ts.entropy_coefficients, s.entropy_coefficient); push!(ts.q_values, s.mean_q_values); push!(ts.learning_rates, alg.learning_rate)
            push!(ts.grad_norms, s.grad_norm)
        end
        append!(ts.fps, T.(fps[1:it[]]))
        DRiL.add_step!(agent, tot[])
        sac_log_stats(h, env, agent.logger)                                                        # log_stats(env, agent.logger), sac.jl:307: once, the iterations ran inside one library call
        GC.@preserve flat tgt begin
            sac_check(ccall((:dril_sac_get_params, LIB[]), Int32, (Ptr{Cvoid}, Ptr{Float32}, Csize_t), h, flat, length(flat)), h)
            sac_check(ccall((:dril_sac_get_target_params, LIB[]), Int32, (Ptr{Cvoid}, Ptr{Float32}, Csize_t), h, tgt, length(tgt)), h)
        end
        sac_scatter_params!(agent.train_state.parameters, flat); sac_scatter_targets!(agent.aux.Q_target_parameters, tgt)
        le = Ref{Float32}(0); sac_check(ccall((:dril_sac_get_log_ent_coef, LIB[]), Int32, (Ptr{Cvoid}, Ref{Float32}), h, le), h)
        agent.aux.ent_train_state.parameters.log_ent_coef[1] = le[]
        !isnothing(callbacks) && all(c -> DRiL.on_training_end(c, Dict{Symbol, Any}(:agent => agent, :env => env, :alg => alg)), callbacks)
        (env.normalize !== nothing && normalization_stats !== nothing) && (normalization_stats[] = sac_norm_stats(h))   # the wrapper lives in the handle: its statistics leave through the Ref
        return agent, nothing, ts, to
    finally
        ccall((:dril_sac_destroy, LIB[]), Int32, (Ptr{Cvoid},), h)
    end
end

# ---- SAC over host envs: train!(agent, OnDevice(env), alg::SAC, max_steps)  (sac.jl:428-559 with the collection loop of off_policy_collection.jl:28-96) ----
function sac_config(w::OnDevice, alg::DRiL.SAC, agent)
    osp, asp = observation_space(w), action_space(w)
    asp isa Box || error("SAC needs a Box action space (sac.jl:74)")
    lo, hi = Float32(minimum(asp.low)), Float32(maximum(asp.high))
    (all(==(lo), asp.low) && all(==(hi), asp.high)) || error("DRIL_ENV_EXTERNAL SAC: one (low, high) pair for all action dimensions (wrap the env in ScalingWrapperEnv)")
    hd = hidden_dims_of(agent.train_state.parameters)
    act = agent.layer.actor_head.layers[1].layers[1].activation === DRiL.Lux.relu ? Int32(1) : Int32(0)
    ec = alg.ent_coef
    auto = ec isa DRiL.AutoEntropyCoefficient
    auto_t = auto && ec.target isa DRiL.AutoEntropyTarget
    return DrilSacConfig(UInt32(1), Int32(5), number_of_envs(w), 0, hd[1], hd[2], act,
        alg.buffer_capacity, alg.start_steps, alg.batch_size, alg.tau, alg.gamma, alg.train_freq, alg.gradient_steps, alg.target_update_interval,
        Int32(auto), auto ? Float32(ec.initial_value) : Float32(ec.coef), Int32(auto ? auto_t : true),
        auto && !auto_t ? Float32(ec.target.target) : 0.0f0,
        alg.learning_rate, 0.9f0, 0.999f0, 1.0f-8, w.seed, w.device, Int32(0),
        Int32(prod(size(osp))), Int32(prod(size(asp))), lo, hi, ntuple(_ -> Int32(0), 4))
end

function train!(agent::SACAgent, w::OnDevice, alg::DRiL.SAC, max_steps::Int; ad_type = nothing, callbacks = nothing)
    T = typeof(alg.learning_rate)
    if has_step_hooks(callbacks)      # on_step hooks: the reference's own loop on the wrapped env
        kw = isnothing(ad_type) ? (; callbacks = callbacks) : (; ad_type = ad_type, callbacks = callbacks)
        return train!(agent, w.env, alg, max_steps; kw...)
    end
    to = TimerOutput()
    cfg = Ref(sac_config(w, alg, agent)); hp = Ref{Ptr{Cvoid}}(C_NULL)
    sac_check(ccall((:dril_sac_create, LIB[]), Int32, (Ref{DrilSacConfig}, Ref{Ptr{Cvoid}}), cfg, hp)); h = hp[]
    try
        flat = sac_flatten_params(agent.train_state.parameters); tgt = sac_flatten_targets(agent.aux.Q_target_parameters)
        GC.@preserve flat tgt begin
            sac_check(ccall((:dril_sac_set_params, LIB[]), Int32, (Ptr{Cvoid}, Ptr{Float32}, Csize_t), h, flat, length(flat)), h)
            sac_check(ccall((:dril_sac_set_target_params, LIB[]), Int32, (Ptr{Cvoid}, Ptr{Float32}, Csize_t), h, tgt, length(tgt)), h)
        end
        sac_check(ccall((:dril_sac_set_log_ent_coef, LIB[]), Int32, (Ptr{Cvoid}, Float32), h, first(agent.aux.ent_train_state.parameters.log_ent_coef)), h)
        E = number_of_envs(w); asp = action_space(w); D = prod(size(observation_space(w))); A = prod(size(asp))
        total_start = alg.start_steps > 0 ? alg.start_steps : alg.train_freq * E                  # sac.jl:456-466
        adjusted = max(1, div(total_start, E)) * E
        n_steps = div(adjusted, E)
        iterations = div(max_steps - adjusted, alg.train_freq * E) + 1
        n_upd = DRiL.get_gradient_steps(alg, alg.train_freq, E)
        ts = DRiL.SACTrainingStats{T}()
        obs = Matrix{Float32}(undef, D, E); nobs = similar(obs); tobs = zeros(Float32, D, E)
        raw = Matrix{Float32}(undef, A, E); ea = similar(raw)
        rew = Vector{Float32}(undef, E); term = Vector{UInt8}(undef, E); trunc = Vector{UInt8}(undef, E)
        st = Vector{DrilSacStats}(undef, max(1, n_upd))
        pack!(dst, xs) = (for j in 1:E; dst[:, j] .= vec(xs[j]); end; dst)
        pack!(obs, observe(w.env))
        @timeit to "training_loop" for it in 1:iterations
            use_random = it == 1 && alg.start_steps > 0                                           # :487
            t0 = time()
            @timeit to "collect_rollout" for _ in 1:n_steps                                       # collect_trajectories, off_policy_collection.jl:28-96
                if use_random
                    for j in 1:E; ea[:, j] .= vec(rand(agent.rng, asp)); end; raw .= ea               # rand(rng, act_space): env space, stored as is (:50-53,72)
                else
                    GC.@preserve obs raw ea sac_check(ccall((:dril_sac_predict_actions, LIB[]), Int32, (Ptr{Cvoid}, Ptr{Float32}, Int64, Int32, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}),
                        h, obs, E, 0, C_NULL, raw, ea), h)                                         # predict_actions_raw + to_env(TanhScaleAdapter), :55-58
                end
                r, te, tr, infos = act!(w.env, [reshape(ea[:, j], size(asp)) for j in 1:E])       # :60
                pack!(nobs, observe(w.env))                                                        # :61
                rew .= r; term .= te; trunc .= tr
                for j in 1:E
                    tr[j] && haskey(infos[j], "terminal_observation") && (tobs[:, j] .= vec(infos[j]["terminal_observation"]))
                end
                GC.@preserve obs raw rew term trunc nobs tobs sac_check(ccall((:dril_sac_ext_push, LIB[]), Int32,
                    (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{UInt8}, Ptr{UInt8}, Ptr{Float32}, Ptr{Float32}), h, obs, raw, rew, term, trunc, nobs, tobs), h)   # push!(buffer, traj), replay_buffer.jl:98-114
                obs, nobs = nobs, obs
            end
            push!(ts.fps, T(n_steps * E / max(time() - t0, 1.0e-12))); DRiL.add_step!(agent, n_steps * E)
            n_steps = alg.train_freq                                                               # :520
            if n_upd > 0
                @timeit to "gradient_updates" GC.@preserve st sac_check(ccall((:dril_sac_update, LIB[]), Int32, (Ptr{Cvoid}, Int32, Ptr{DrilSacStats}), h, n_upd, st), h)   # :523-538
                for k in 1:n_upd
                    s = st[k]
                    push!(ts.actor_losses, s.actor_loss); push!(ts.critic_losses, s.critic_loss); s.has_entropy_loss != 0 && push!(ts.entropy_losses, s.entropy_loss)
                    push!(ts.entropy_coefficients, s.entropy_coefficient); push!(ts.q_values, s.mean_q_values); push!(ts.learning_rates, alg.learning_rate)
                    push!(ts.grad_norms, s.grad_norm)
                end
            end
        end
        GC.@preserve flat tgt begin
            sac_check(ccall((:dril_sac_get_params, LIB[]), Int32, (Ptr{Cvoid}, Ptr{Float32}, Csize_t), h, flat, length(flat)), h)
            sac_check(ccall((:dril_sac_get_target_params, LIB[]), Int32, (Ptr{Cvoid}, Ptr{Float32}, Csize_t), h, tgt, length(tgt)), h)
        end
        sac_scatter_params!(agent.train_state.parameters, flat); sac_scatter_targets!(agent.aux.Q_target_parameters, tgt)
        le = Ref{Float32}(0); sac_check(ccall((:dril_sac_get_log_ent_coef, LIB[]), Int32, (Ptr{Cvoid}, Ref{Float32}), h, le), h)
        agent.aux.ent_train_state.parameters.log_ent_coef[1] = le[]
        return agent, nothing, ts, to
    finally
        ccall((:dril_sac_destroy, LIB[]), Int32, (Ptr{Cvoid},), h)
    end
end

# ---- the same loop on DEVICE arrays (DRIL_ENV_EXTERNAL; include/dril_sac.h, docs/sac.md last section) ------------------------------------------------------
# Thin wrappers of the sync-free verbs for a simulator whose batched arrays already live on the GPU (AMDGPU.jl ROCArrays: pass `pointer(x)` converted to Ptr{Cvoid}).
# `h` is a dril_sac_handle* of dril_sac_create with DRIL_ENV_EXTERNAL; `stream` a hipStream_t (C_NULL: the null stream).  None of act / push / predict / enqueue
# waits on the host; sac_flush! is the one drain and returns the pending statistics rows.
struct DrilSacExtDeviceInfo
    steps_device::Int64; steps_host::Int64; host_syncs::Int64; flushes::Int64; launches::Int64
    pending_updates::Int32; pending_capacity::Int32; per_dim_bounds::Int32
    reserved::NTuple{5, Int32}
end
const SAC_PENDING_CAPACITY = 4096
sac_ext_act_device!(h, d_obs, use_random::Bool, d_noise, d_stored, d_env_actions, stream = C_NULL) =
    sac_check(ccall((:dril_sac_ext_act_device, LIB[]), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                    h, d_obs, Int32(use_random), d_noise, d_stored, d_env_actions, stream), h)
sac_ext_push_device!(h, d_rewards, d_terminated, d_truncated, d_next_obs, d_terminal_obs = C_NULL, stream = C_NULL) =
    sac_check(ccall((:dril_sac_ext_push_device, LIB[]), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                    h, d_rewards, d_terminated, d_truncated, d_next_obs, d_terminal_obs, stream), h)
sac_predict_actions_device!(h, d_obs, batch::Integer, deterministic::Bool, d_noise, d_raw_actions, d_env_actions, stream = C_NULL) =
    sac_check(ccall((:dril_sac_predict_actions_device, LIB[]), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int32, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                    h, d_obs, Int64(batch), Int32(deterministic), d_noise, d_raw_actions, d_env_actions, stream), h)
sac_update_enqueue!(h, n_updates::Integer) = sac_check(ccall((:dril_sac_update_enqueue, LIB[]), Int32, (Ptr{Cvoid}, Int32), h, Int32(n_updates)), h)
function sac_flush!(h)
    st = Vector{DrilSacStats}(undef, SAC_PENDING_CAPACITY); n = Ref{Int64}(0)
    GC.@preserve st sac_check(ccall((:dril_sac_flush, LIB[]), Int32, (Ptr{Cvoid}, Ptr{DrilSacStats}, Int64, Ref{Int64}), h, st, Int64(length(st)), n), h)
    return st[1:n[]]
end
function sac_ext_set_action_bounds!(h, low::Vector{Float32}, high::Vector{Float32})
    GC.@preserve low high sac_check(ccall((:dril_sac_ext_set_action_bounds, LIB[]), Int32, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}), h, low, high), h)
end
function sac_ext_device_info(h)
    info = Ref{DrilSacExtDeviceInfo}()
    sac_check(ccall((:dril_sac_ext_device_info, LIB[]), Int32, (Ptr{Cvoid}, Ref{DrilSacExtDeviceInfo}), h, info), h)
    return info[]
end

# ---- NormalizeWrapperEnv / MonitorWrapperEnv around such envs (dril_sac_ext_normalize_* / dril_sac_ext_monitor_*, include/dril_sac.h) ----------------------------
# The device verbs above honour them and stay free of host waits.  sac_ext_collection_begin! marks the next sac_ext_act_device! as the opening observe(env) of a
# collect_trajectories call (off_policy_collection.jl:43): call it before every collection while the normaliser is on.
struct DrilSacExtWrapInfo                                                # struct dril_sac_ext_wrap_info
    normalize_on::Int32; monitor_on::Int32; monitor_window::Int32; reserved0::Int32
    launches_act::Int64; launches_push::Int64; allocations::Int64
    reserved::NTuple{3, Int64}
end
function sac_ext_normalize_enable!(h::Ptr{Cvoid}, nz::Union{Nothing, NamedTuple})
    isnothing(nz) && return sac_check(ccall((:dril_sac_ext_normalize_enable, LIB[]), Int32, (Ptr{Cvoid}, Ptr{Cvoid}), h, C_NULL), h)
    g(k, d) = get(nz, k, d)
    cfg = Ref(DrilSacNormalizeConfig(Int32(g(:training, true)), Int32(g(:norm_obs, true)), Int32(g(:norm_reward, true)),
        Float32(g(:clip_obs, 10.0f0)), Float32(g(:clip_reward, 10.0f0)), Float32(g(:gamma, 0.99f0)), Float32(g(:epsilon, 1.0f-8)), Int32(0)))
    return sac_check(ccall((:dril_sac_ext_normalize_enable, LIB[]), Int32, (Ptr{Cvoid}, Ref{DrilSacNormalizeConfig}), h, cfg), h)
end
function sac_ext_normalize_config(h::Ptr{Cvoid})
    cfg = Ref{DrilSacNormalizeConfig}()
    sac_check(ccall((:dril_sac_ext_normalize_get_config, LIB[]), Int32, (Ptr{Cvoid}, Ref{DrilSacNormalizeConfig}), h, cfg), h)
    return cfg[]
end
sac_ext_normalize_set_training!(h::Ptr{Cvoid}, training::Bool) =
    sac_check(ccall((:dril_sac_ext_normalize_set_training, LIB[]), Int32, (Ptr{Cvoid}, Int32), h, Int32(training)), h)
function sac_ext_normalize_get_stats(h::Ptr{Cvoid}, D::Integer)
    om = Vector{Float32}(undef, D); ov = Vector{Float32}(undef, D); oc = Ref{Int64}(0); rc = Ref{Int64}(0); rm = Ref{Float32}(0); rv = Ref{Float32}(0)
    GC.@preserve om ov sac_check(ccall((:dril_sac_ext_normalize_get_stats, LIB[]), Int32, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ref{Int64}, Ref{Float32}, Ref{Float32}, Ref{Int64}),
                                       h, om, ov, oc, rm, rv, rc), h)
    return (obs_mean = om, obs_var = ov, obs_count = oc[], ret_mean = rm[], ret_var = rv[], ret_count = rc[])
end
function sac_ext_normalize_set_stats!(h::Ptr{Cvoid}, st)
    om = Vector{Float32}(st.obs_mean); ov = Vector{Float32}(st.obs_var)
    GC.@preserve om ov sac_check(ccall((:dril_sac_ext_normalize_set_stats, LIB[]), Int32, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Int64, Float32, Float32, Int64),
                                       h, om, ov, Int64(st.obs_count), Float32(st.ret_mean), Float32(st.ret_var), Int64(st.ret_count)), h)
end
function sac_ext_normalize_get_original(h::Ptr{Cvoid}, E::Integer, D::Integer)
    obs = Matrix{Float32}(undef, D, E); rew = Vector{Float32}(undef, E)
    GC.@preserve obs rew sac_check(ccall((:dril_sac_ext_normalize_get_original, LIB[]), Int32, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}), h, obs, rew), h)
    return obs, rew
end
function sac_ext_normalize_get_returns(h::Ptr{Cvoid}, E::Integer)
    r = Vector{Float32}(undef, E)
    GC.@preserve r sac_check(ccall((:dril_sac_ext_normalize_get_returns, LIB[]), Int32, (Ptr{Cvoid}, Ptr{Float32}), h, r), h)
    return r
end
sac_ext_normalize_reset!(h::Ptr{Cvoid}, stream = C_NULL) = sac_check(ccall((:dril_sac_ext_normalize_reset, LIB[]), Int32, (Ptr{Cvoid}, Ptr{Cvoid}), h, stream), h)
sac_ext_collection_begin!(h::Ptr{Cvoid}) = sac_check(ccall((:dril_sac_ext_collection_begin, LIB[]), Int32, (Ptr{Cvoid},), h), h)
sac_ext_monitor_enable!(h::Ptr{Cvoid}, window::Integer) = sac_check(ccall((:dril_sac_ext_monitor_enable, LIB[]), Int32, (Ptr{Cvoid}, Int32), h, Int32(window)), h)
function sac_ext_monitor_stats(h::Ptr{Cvoid})
    r = Ref{Float32}(NaN32); l = Ref{Float32}(NaN32); n = Ref{Int32}(0)
    sac_check(ccall((:dril_sac_ext_monitor_get_stats, LIB[]), Int32, (Ptr{Cvoid}, Ref{Float32}, Ref{Float32}, Ref{Int32}), h, r, l, n), h)
    return (ep_rew_mean = r[], ep_len_mean = l[], n_episodes = n[])
end
function sac_ext_wrap_info(h::Ptr{Cvoid})
    info = Ref{DrilSacExtWrapInfo}()
    sac_check(ccall((:dril_sac_ext_wrap_info, LIB[]), Int32, (Ptr{Cvoid}, Ref{DrilSacExtWrapInfo}), h, info), h)
    return info[]
end
