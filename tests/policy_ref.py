"""float64 NumPy restatement of a deployment policy (include/dril_policy.h): normalise -> MLP (the eight activations) -> distribution head -> action adapter.
Independent of the library: the GPU tests compare policy_act_kernel against these lines."""
import numpy as np

ACTIVATIONS = ("tanh", "relu", "sigmoid", "elu", "leakyrelu", "softplus", "gelu", "swish")


def activation(name, x):
    x = np.asarray(x, np.float64)
    if name == "tanh":
        return np.tanh(x)
    if name == "relu":
        return np.maximum(x, 0.0)
    if name == "sigmoid":
        return 1.0 / (1.0 + np.exp(-x))
    if name == "elu":
        return np.where(x > 0, x, np.expm1(np.minimum(x, 0.0)))
    if name == "leakyrelu":
        return np.where(x > 0, x, 0.01 * x)
    if name == "softplus":
        return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))
    if name == "gelu":                                                       # NNlib.gelu, the tanh form
        return 0.5 * x * (1.0 + np.tanh(np.sqrt(2.0 / np.pi) * (x + 0.044715 * x ** 3)))
    if name == "swish":
        return x / (1.0 + np.exp(-x))
    raise ValueError(name)


def normalize(obs, mean, var, eps, clip):
    """normalize_obs!, normalizeWrapperEnv.jl:174-179"""
    return np.clip((np.asarray(obs, np.float64) - np.asarray(mean, np.float64)) / np.sqrt(np.asarray(var, np.float64) + eps), -clip, clip)


def random_actor(rng, dims, scale=1.0):
    """[(W (out x in), b)] per layer, float32"""
    return [((rng.standard_normal((o, i)) * scale / np.sqrt(i)).astype(np.float32), (rng.standard_normal(o) * 0.1).astype(np.float32))
            for i, o in zip(dims[:-1], dims[1:])]


def flat_actor(layers):
    """the actor's slice of dril_get_params: W column-major (out x in), then b, layer by layer"""
    return np.concatenate([np.concatenate([W.ravel(order="F"), b]) for W, b in layers]).astype(np.float32)


def mlp(layers, x, act):
    """x (B, D) -> (B, out): Dense(in => h, act) ... Dense(h => out)"""
    h = np.asarray(x, np.float64)
    for l, (W, b) in enumerate(layers):
        h = h @ W.astype(np.float64).T + b.astype(np.float64)
        if l + 1 < len(layers):
            h = activation(act, h)
    return h


def softmax(z):
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def categorical(z, deterministic, u=None, action_start=1):
    """-> (actions, margin): deterministic: the logit margin between the two best actions; sampled: the distance of u from the nearest CDF step"""
    p = softmax(z)
    if deterministic:
        srt = np.sort(z, axis=1)
        return p.argmax(axis=1) + action_start, (srt[:, -1] - srt[:, -2] if z.shape[1] > 1 else np.full(len(z), np.inf))
    cs = np.cumsum(p, axis=1)
    a = np.array([min(int(np.searchsorted(c, ui, side="left")), len(c) - 1) for c, ui in zip(cs, u)])     # findfirst(cumsum(p) .>= u)
    return a + action_start, np.abs(cs - np.asarray(u)[:, None]).min(axis=1)


def diag_gaussian(mu, log_std, deterministic, noise, low, high):
    """-> (raw, env): DiagGaussian + ClampAdapter; low >= high in a dimension: no clamp there"""
    raw = mu if deterministic else mu + np.exp(np.asarray(log_std, np.float64)) * noise
    low, high = np.asarray(low, np.float64), np.asarray(high, np.float64)
    return raw, np.where(low < high, np.minimum(np.maximum(raw, low), np.maximum(high, low)), raw)


def squashed(mu, log_std, deterministic, noise, low, high):
    """-> (raw, env): SquashedDiagGaussian + TanhScaleAdapter, which squashes again (default_adapters.jl:13-21)"""
    raw = np.tanh(mu if deterministic else mu + np.exp(np.asarray(log_std, np.float64)) * noise)
    low, high = np.asarray(low, np.float64), np.asarray(high, np.float64)
    return raw, np.tanh(raw) * (high - low) / 2.0 + (low + high) / 2.0
