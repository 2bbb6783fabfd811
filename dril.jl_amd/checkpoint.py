"""Checkpoint round trip in the reference's key schema (host-side data only; no device code).

    save_policy_params_and_state(agent, path)          src/agents/agent_methods.jl:122-138   keys: layer, parameters, states, aux
    load_policy_params_and_state_(agent, alg, path)    src/algorithms/ppo.jl:77-94           (the optimiser state is rebuilt, not loaded)
    save_normalization_stats / load_normalization_stats_   src/environment_wrappers/normalizeWrapperEnv.jl:261-297
                                                       keys: obs_mean obs_var obs_count ret_mean ret_var ret_count clip_obs clip_reward gamma epsilon
    save_policy(policy, path) / load_policy(path)      a deployment policy (deployment.py) in ONE file: descriptor fields under policy/, the actor tree under
                                                       parameters/actor_head/layer_k/{weight,bias} (+ parameters/log_std), obs_mean / obs_var when it carries statistics

The reference writes JLD2 (Julia objects); a Julia user keeps doing exactly that on `agent.train_state.parameters`, which DRiLHIP.jl's
`train!` fills with the device-trained weights.  This Python mirror stores the same keys in an `.npz`, leaves flattened
with "/" paths (`parameters/actor_head/layer_1/weight`, `aux/Q_target_parameters`, ...), so the two files can be converted key by key.
"""
from __future__ import annotations

import json
from dataclasses import asdict, is_dataclass
from pathlib import Path

import numpy as np


def _flatten(prefix: str, tree, out: dict):
    if isinstance(tree, dict):
        for k, v in tree.items():
            _flatten(f"{prefix}/{k}", v, out)
    else:
        out[prefix] = np.asarray(tree)


def _unflatten(prefix: str, data) -> dict:
    tree: dict = {}
    for key in data.files:
        if not key.startswith(prefix + "/"):
            continue
        node = tree
        parts = key[len(prefix) + 1:].split("/")
        for p in parts[:-1]:
            node = node.setdefault(p, {})
        node[parts[-1]] = data[key]
    return tree


def _layer_desc(layer) -> str:
    d = {k: v for k, v in asdict(layer).items() if k not in ("observation_space", "action_space")} if is_dataclass(layer) else {}
    d["type"] = type(layer).__name__
    d["hidden_dims"] = list(getattr(layer, "hidden_dims", ()))
    return json.dumps(d, default=lambda o: list(o) if isinstance(o, (tuple, np.ndarray)) else str(o))


def save_policy_params_and_state(agent, path, suffix: str = ".npz") -> str:
    """agent: Agent (PPO) or SACAgent.  -> file path"""
    file_path = str(path) if str(path).endswith(suffix) else str(path) + suffix
    out = {"layer": np.array(_layer_desc(agent.layer))}
    params = agent.train_state.parameters if hasattr(agent, "train_state") else agent.parameters
    _flatten("parameters", params, out)
    out["states"] = np.array("{}")                                      # the MLPs carry no Lux state (NamedTuple())
    if hasattr(agent, "q_target_parameters"):                           # QAux, sac.jl:172-178
        out["aux/Q_target_parameters"] = np.asarray(agent.q_target_parameters)
        out["aux/log_ent_coef"] = np.asarray([agent.log_ent_coef], np.float32)
    np.savez(file_path, **out)
    return file_path


def load_policy_params_and_state_(agent, alg, path, suffix: str = ".npz"):
    """load_policy_params_and_state!(agent, alg, path) (ppo.jl:77-94): parameters and aux replace the agent's and a NEW TrainState is built
    (`Lux.Training.TrainState(layer, parameters, states, make_optimizer(alg))` :88-91) — the Adam moments are not restored: the new TrainState carries
    optimizer_state = None and the next train_ starts from zero moments on whatever env it runs.  `agent.layer = data["layer"]` (ppo.jl:90): the stored layer
    description must describe the agent's layer — a checkpoint of another architecture raises instead of loading into mismatched shapes"""
    file_path = str(path) if str(path).endswith(suffix) else str(path) + suffix
    data = np.load(file_path, allow_pickle=False)
    params = _unflatten("parameters", data)
    stored, mine = json.loads(str(data["layer"])), json.loads(_layer_desc(agent.layer))
    for k in ("type", "hidden_dims", "activation"):
        if k in stored and k in mine and stored[k] != mine[k]:
            raise ValueError(f"checkpoint {file_path} was written for a layer with {k} = {stored[k]!r}; this agent's layer has {mine[k]!r} (ppo.jl:90 replaces agent.layer with the stored one)")
    if hasattr(agent, "train_state"):
        agent.train_state = type(agent.train_state)(parameters=params, step=0)
    else:
        agent.parameters = params
    if "aux/Q_target_parameters" in data.files:
        agent.q_target_parameters = data["aux/Q_target_parameters"].copy()
        agent.log_ent_coef = float(data["aux/log_ent_coef"][0])
    agent.alg = alg
    return agent


_NORM_KEYS = ("obs_mean", "obs_var", "obs_count", "ret_mean", "ret_var", "ret_count")


def _norm_handle_kw(env):
    """(the object with norm_get_stats / norm_set_stats, the wrapper's keywords or None): a DeviceParallelEnv with NormalizeWrapperEnv and a bound PPO handle, or a
    SacHandle with the wrapper on (dril_sac_normalize_enable) — `replay_buffer.handle` after sac_train_"""
    from .host import _env_handle, _norm_view, _normalize_kw               # an external handle's wrapper answers through dril_ext_normalize_* / dril_sac_ext_normalize_*
    if hasattr(env, "norm_get_stats"):
        return _norm_view(env), None
    return _norm_view(_env_handle(env)), _normalize_kw(env)


def save_normalization_stats(env, filepath, **keywords) -> str:
    """env: a DeviceParallelEnv with NormalizeWrapperEnv switched on and a bound handle, or a SacHandle with the wrapper on (clip_obs / clip_reward / gamma /
    epsilon are read from the handle: dril_sac_normalize_get_config; keywords override).  File keys: those of save_normalization_stats, normalizeWrapperEnv.jl:261-277"""
    h, kw = _norm_handle_kw(env)
    if kw is None and hasattr(h, "normalize_config"):
        kw = h.normalize_config()                                      # a SacHandle holds the wrapper's keywords itself
    kw = {**dict(clip_obs=10.0, clip_reward=10.0, gamma=0.99, epsilon=1e-8), **(kw or {}), **keywords}
    st = h.norm_get_stats()
    fp = str(filepath) if str(filepath).endswith(".npz") else str(filepath) + ".npz"
    np.savez(fp, **{k: np.asarray(st[k]) for k in _NORM_KEYS}, clip_obs=kw["clip_obs"], clip_reward=kw["clip_reward"], gamma=kw["gamma"], epsilon=kw["epsilon"])
    return fp


def load_normalization_stats_(env, filepath):
    fp = str(filepath) if str(filepath).endswith(".npz") else str(filepath) + ".npz"
    d = np.load(fp)
    h, _ = _norm_handle_kw(env)
    h.norm_set_stats(d["obs_mean"], d["obs_var"], int(d["obs_count"]), float(d["ret_mean"]), float(d["ret_var"]), int(d["ret_count"]))
    return env


_POLICY_FIELDS = ("kind", "obs_dim", "action_dim", "action_start", "activation", "has_norm", "clip_obs", "epsilon")


def policy_file_dict(desc, actor_flat, log_std=None, obs_mean=None, obs_var=None) -> dict:
    """the arrays save_policy stores (host data only): the descriptor of include/dril_policy.h field by field, the actor in the parameter key schema, the statistics"""
    from .deployment import actor_flat_to_tree
    A, nh = desc.action_dim, desc.n_hidden
    hidden = [int(desc.hidden[l]) for l in range(nh)]
    out = {f"policy/{k}": np.asarray(getattr(desc, k)) for k in _POLICY_FIELDS}
    out["policy/hidden_dims"] = np.asarray(hidden, np.int32)
    out["policy/action_low"] = np.asarray([desc.action_low[a] for a in range(A)], np.float32)
    out["policy/action_high"] = np.asarray([desc.action_high[a] for a in range(A)], np.float32)
    _flatten("parameters/actor_head", actor_flat_to_tree(np.asarray(actor_flat, np.float32), (desc.obs_dim, *hidden, A)), out)
    if log_std is not None:
        out["parameters/log_std"] = np.asarray(log_std, np.float32)
    if desc.has_norm:
        out["obs_mean"], out["obs_var"] = np.asarray(obs_mean, np.float32), np.asarray(obs_var, np.float32)
    return out


def policy_from_file_dict(data, device: int = 0):
    """-> (descriptor, actor parameters flat, log_std | None, obs_mean | None, obs_var | None): the arguments of NeuralPolicy.create"""
    from .deployment import actor_tree_to_flat, make_policy_desc
    g = lambda k: data["policy/" + k]
    has_norm = bool(int(g("has_norm")))
    desc = make_policy_desc(int(g("kind")), int(g("obs_dim")), int(g("action_dim")), [int(h) for h in g("hidden_dims")], int(g("activation")),
                            action_start=int(g("action_start")), action_low=g("action_low"), action_high=g("action_high"),
                            clip_obs=float(g("clip_obs")) if has_norm else None, epsilon=float(g("epsilon")), device=device)
    tree = _unflatten("parameters", data)
    return (desc, actor_tree_to_flat(tree["actor_head"]), tree.get("log_std"), data["obs_mean"] if has_norm else None, data["obs_var"] if has_norm else None)


def save_policy(policy, path, suffix: str = ".npz") -> str:
    """a NeuralPolicy / NormWrapperPolicy -> one .npz: enough to deploy on a machine that never saw the training run"""
    file_path = str(path) if str(path).endswith(suffix) else str(path) + suffix
    flat, log_std = policy.get_params()
    mean, var = policy.get_norm() if policy.desc.has_norm else (None, None)
    np.savez(file_path, **policy_file_dict(policy.desc, flat, log_std, mean, var))
    return file_path


def load_policy(path, device: int = 0, suffix: str = ".npz"):
    from .deployment import NeuralPolicy
    file_path = str(path) if str(path).endswith(suffix) else str(path) + suffix
    return NeuralPolicy.create(*policy_from_file_dict(np.load(file_path, allow_pickle=False), device))
