"""CPU: the deployment-policy surface that needs no GPU — the C ABI of include/dril_policy.h against the library and the ctypes mirror, RandomPolicy /
ConstantPolicy, the shape rule of policy calls, the save_policy / load_policy file (host arrays), the Julia shim's ccall sites."""
import ctypes as C
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import policy_ref

ROOT = Path(__file__).resolve().parents[1]


def test_policy_symbols_are_declared_exported_and_typed(pkg):
    header = (ROOT / "include" / "dril_policy.h").read_text()
    declared = set(re.findall(r"\b(dril_policy_[a-z0-9_]+)\s*\(", header))
    assert {"dril_policy_create", "dril_policy_from_handle", "dril_policy_from_sac_handle", "dril_policy_act", "dril_policy_describe", "dril_policy_get_params",
            "dril_policy_get_norm", "dril_policy_set_seed", "dril_policy_destroy", "dril_policy_last_error"} <= declared
    assert declared == {s for s in pkg._capi.EXPORTED_SYMBOLS if s.startswith("dril_policy_")} - {"dril_policy_forward"}   # (dril_hip.h: the training handle's forward)
    so = ROOT / "dril.jl_amd" / "csrc" / "libdril_hip.so"
    out = subprocess.run(["nm", "-D", "--defined-only", str(so)], capture_output=True, text=True, check=True).stdout
    assert declared <= set(re.findall(r" T (dril_policy_[a-z0-9_]+)", out))
    lib = pkg._capi.load_library()
    assert lib.dril_policy_param_count(None) == -1


def test_policy_desc_layout_matches_c(pkg, tmp_path):
    fields = [n for n, _ in pkg._capi.DrilPolicyDesc._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dril_policy.h"\nint main(){printf("%zu", sizeof(dril_policy_desc));\n'
                   + "".join(f'printf(" %zu", offsetof(dril_policy_desc, {f}));\n' for f in fields) + 'printf("\\n");return 0;}')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    K = pkg._capi.DrilPolicyDesc
    assert got == [C.sizeof(K)] + [getattr(K, f).offset for f in fields]


def test_bad_descriptors_are_refused_before_any_device_call(pkg):
    lib, cap = pkg._capi.load_library(), pkg._capi
    mk = pkg.deployment.make_policy_desc
    flat = np.zeros(8, np.float32)
    for desc, word in ((mk(0, 4, 2, (8, 8, 8, 8, 8), "tanh"), b"n_hidden"), (mk(0, 4, 2, (1025,), "tanh"), b"1..1024"), (mk(0, 1025, 2, (8,), "tanh"), b"obs_dim"),
                       (mk(1, 4, 65, (8,), "tanh"), b"action_dim"), (mk(3, 4, 2, (8,), "tanh"), b"kind"), (mk(0, 4, 2, (8,), 9), b"activation")):
        p = C.c_void_p()
        assert lib.dril_policy_create(C.byref(desc), flat.ctypes.data_as(C.c_void_p), flat.size, None, None, None, C.byref(p)) == cap.ERR_INVALID_ARG
        assert word in lib.dril_policy_last_error(None) and not p.value
    good, p = mk(0, 4, 2, (8,), "tanh"), C.c_void_p()
    assert lib.dril_policy_create(C.byref(good), flat.ctypes.data_as(C.c_void_p), 7, None, None, None, C.byref(p)) == cap.ERR_INVALID_ARG   # 4*8+8 + 8*2+2 = 58
    assert b"58" in lib.dril_policy_last_error(None)
    assert lib.dril_policy_create(C.byref(good), None, 58, None, None, None, C.byref(p)) == cap.ERR_INVALID_ARG
    assert lib.dril_policy_act(None, None, 1, 1, None, None, None) == cap.ERR_NOT_INITIALISED
    assert lib.dril_policy_destroy(None) == cap.ERR_NOT_INITIALISED


def test_random_policy_bounds_and_rng(pkg):
    box = pkg.Box((-2.0, 0.5, -1.0), (2.0, 0.75, 3.0))
    rp = pkg.RandomPolicy(box)
    draws = np.stack([rp(None, rng=np.random.default_rng(s)) for s in range(200)])
    assert draws.dtype == np.float32 and (draws >= np.asarray(box.low, np.float32)).all() and (draws <= np.asarray(box.high, np.float32)).all()
    assert draws.std(axis=0).min() > 0.01
    assert np.array_equal(rp(None, rng=np.random.default_rng(5)), rp(None, rng=np.random.default_rng(5)))
    g = np.random.default_rng(6)
    assert not np.array_equal(rp(None, rng=g), rp(None, rng=g))
    dp = pkg.RandomPolicy(pkg.CartPoleEnv())                              # RandomPolicy(env) takes the env's action space
    acts = {dp(np.zeros(4), rng=np.random.default_rng(s)) for s in range(64)}
    assert acts == {1, 2}
    assert {pkg.RandomPolicy(pkg.Discrete(3, 0))(None, rng=np.random.default_rng(s)) for s in range(64)} == {0, 1, 2}


def test_constant_policy(pkg):
    a = np.array([0.25], np.float32)
    cp = pkg.ConstantPolicy(a)
    assert cp(np.zeros(3)) is a and cp([np.zeros(3)] * 4, deterministic=True) is a
    with pytest.raises(ValueError, match="deterministic"):
        cp(np.zeros(3), deterministic=False)
    with pytest.warns(UserWarning, match="rng"):
        cp(np.zeros(3), rng=np.random.default_rng(0))


class _Stub:
    """the host half of a NeuralPolicy call: records what `act` receives"""
    def __init__(self, discrete, A=2):
        self.discrete, self.A, self.calls = discrete, A, []

    def act(self, obs, deterministic, noise):
        self.calls.append((obs.copy(), deterministic, None if noise is None else noise.copy()))
        return np.arange(len(obs), dtype=np.int32) + 1 if self.discrete else np.tile(obs[:, :1], (1, self.A)).astype(np.float32)

    _draw = lambda self, rng, B: (rng.random(B) if self.discrete else rng.standard_normal((B, self.A)).astype(np.float32))
    _format = lambda self, row: (int(row) if self.discrete else row)


def test_shape_rule_single_vs_batch(pkg):
    call = pkg.deployment._call_with_shape_rule
    st = _Stub(True)
    one = call(st, np.zeros(4, np.float32), True, None)
    assert isinstance(one, int) and one == 1 and st.calls[-1][0].shape == (1, 4) and st.calls[-1][2] is None
    many = call(st, [np.zeros(4), np.ones(4), np.ones(4)], True, None)
    assert many == [1, 2, 3] and st.calls[-1][0].shape == (3, 4)
    assert call(st, np.zeros((5, 4), np.float32), True, None) == [1, 2, 3, 4, 5]
    assert call(st, [np.zeros(4)], True, None) == [1]                      # a list of one observation is a batch of one
    sb = _Stub(False, A=3)
    act = call(sb, np.full(6, 0.5, np.float32), False, np.random.default_rng(3))
    assert act.shape == (3,) and sb.calls[-1][1] is False
    np.testing.assert_array_equal(sb.calls[-1][2], np.random.default_rng(3).standard_normal((1, 3)).astype(np.float32))   # the rng's draws are what is injected
    call(st, np.zeros((2, 4)), False, np.random.default_rng(4))
    np.testing.assert_array_equal(st.calls[-1][2], np.random.default_rng(4).random(2))
    call(st, np.zeros((2, 4)), True, np.random.default_rng(4))
    assert st.calls[-1][2] is None                                         # deterministic: nothing is drawn


def test_policy_file_round_trip_host_arrays(pkg, tmp_path):
    ck, dep = pkg.checkpoint, pkg.deployment
    rng = np.random.default_rng(0)
    dims = (5, 12, 7, 3)
    layers = policy_ref.random_actor(rng, dims)
    flat, ls = policy_ref.flat_actor(layers), rng.standard_normal(3).astype(np.float32)
    mean, var = rng.standard_normal(5).astype(np.float32), rng.random(5).astype(np.float32) + 0.5
    desc = dep.make_policy_desc(1, 5, 3, dims[1:-1], "gelu", action_low=(-1, -2, 0), action_high=(1, 2, 0), clip_obs=7.5, epsilon=1e-6)
    d = ck.policy_file_dict(desc, flat, ls, mean, var)
    np.testing.assert_array_equal(d["parameters/actor_head/layer_2/weight"], layers[1][0])         # the existing key schema, weights (out x in)
    np.testing.assert_array_equal(d["parameters/actor_head/layer_3/bias"], layers[2][1])
    np.savez(tmp_path / "p.npz", **d)
    desc2, flat2, ls2, mean2, var2 = ck.policy_from_file_dict(np.load(tmp_path / "p.npz", allow_pickle=False))
    assert bytes(desc2) == bytes(desc)
    for a, b in ((flat2, flat), (ls2, ls), (mean2, mean), (var2, var)):
        np.testing.assert_array_equal(a, b)
    cat = dep.make_policy_desc(0, 4, 2, (64, 64), "tanh", action_start=1)
    l2 = policy_ref.random_actor(rng, (4, 64, 64, 2))
    d2 = ck.policy_file_dict(cat, policy_ref.flat_actor(l2))
    assert "parameters/log_std" not in d2 and "obs_mean" not in d2
    np.savez(tmp_path / "c.npz", **d2)
    desc3, flat3, ls3, mean3, var3 = ck.policy_from_file_dict(np.load(tmp_path / "c.npz"))
    assert bytes(desc3) == bytes(cat) and ls3 is None and mean3 is None and np.array_equal(flat3, policy_ref.flat_actor(l2))


def test_policy_ref_is_self_consistent():
    x = np.linspace(-4, 4, 33)
    for name in policy_ref.ACTIVATIONS:
        y = policy_ref.activation(name, x)
        assert y.shape == x.shape and np.isfinite(y).all()
    assert policy_ref.activation("gelu", np.array([0.0]))[0] == 0.0 and abs(policy_ref.activation("softplus", np.array([0.0]))[0] - np.log(2)) < 1e-15
    z = np.array([[0.0, 1.0, 3.0]])
    a, m = policy_ref.categorical(z, True)
    assert a[0] == 3 and m[0] == 2.0
    p = policy_ref.softmax(z)[0]
    assert policy_ref.categorical(z, False, [p[0] * 0.5])[0][0] == 1 and policy_ref.categorical(z, False, [p[0] + p[1] * 0.5])[0][0] == 2
    raw, env = policy_ref.diag_gaussian(np.array([[3.0, -3.0]]), [0.0, 0.0], True, None, [-1.0, 0.0], [1.0, 0.0])
    assert env.tolist() == [[1.0, -3.0]]                                   # low >= high: no clamp in that dimension


def test_shim_declares_the_policy_ccalls():
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "check_shim.py")], capture_output=True, text=True)
    assert r.returncode == 0 and "check_shim: ok" in r.stdout, r.stdout + r.stderr
    extras = (ROOT / "dril.jl_amd" / "julia" / "DRiLHIP_extras.jl").read_text()
    for sym in ("dril_policy_from_handle", "dril_policy_from_sac_handle", "dril_policy_act", "dril_policy_destroy"):
        assert f"(:{sym}, LIB[])" in extras
    assert "struct DevicePolicy" in extras and "function extract_device_policy" in extras
