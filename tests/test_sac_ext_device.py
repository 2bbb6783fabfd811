"""CPU: the device-array verbs of a DRIL_ENV_EXTERNAL SAC handle (dril_sac_ext_act_device / _push_device, dril_sac_predict_actions_device,
dril_sac_update_enqueue / dril_sac_flush, dril_sac_ext_set_action_bounds, dril_sac_ext_device_info; docs/sac.md last section), without a GPU.

  * header prototypes, ctypes declarations and the Julia ccalls agree (tools/check_shim.py's own check functions; a C compile against include/dril_sac.h);
  * the info struct's ctypes layout is the header's;
  * the NumPy restatement of rand(action_space) stays inside the Box at both ends of the uniform's range;
  * every new verb on a null handle returns DRIL_ERR_NOT_INITIALISED before any HIP call;
  * the Python argument checks name the argument before the library is called."""
import ctypes as C
import importlib.util
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
VERBS = ("dril_sac_ext_act_device", "dril_sac_ext_push_device", "dril_sac_predict_actions_device", "dril_sac_update_enqueue", "dril_sac_flush",
         "dril_sac_ext_set_action_bounds", "dril_sac_ext_device_info")
FIELDS = ("steps_device", "steps_host", "host_syncs", "flushes", "launches", "pending_updates", "pending_capacity", "per_dim_bounds", "reserved")


def _check_shim():
    spec = importlib.util.spec_from_file_location("check_shim", ROOT / "tools" / "check_shim.py")
    m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
    return m


def test_header_ctypes_and_julia_agree(pkg, capsys):
    cs = _check_shim()
    assert cs.check_abi() == [] and cs.check_ccalls() == [] and cs.check_blocks() == []
    capsys.readouterr()
    protos = cs.c_prototypes()
    shim = cs.read_shim(cs.SHIM)
    capi = pkg._capi
    for name in VERBS:
        assert name in protos, name
        assert f"(:{name}, LIB[])" in shim, f"no ccall of {name} in the Julia shim"
        res, args = capi._SIG[name]
        assert res is C.c_int32 and len(args) == len(protos[name][1]), (name, args, protos[name][1])
        for k, (ct, cparam) in enumerate(zip(args, protos[name][1])):               # pointer-ness and scalar width of every argument
            kind = cs.c_class(cparam)
            if kind[0] == "ptr":
                assert ct is C.c_void_p or hasattr(ct, "contents") or issubclass(ct, C._Pointer), (name, k, cparam)
            else:
                assert C.sizeof(ct) == kind[1] and ct in (C.c_int32, C.c_int64), (name, k, cparam)
    header = (ROOT / "include" / "dril_sac.h").read_text()
    assert "#define DRIL_SAC_ABI_VERSION 1u" in header and capi.SAC_ABI_VERSION == 1                                # only new symbols: the ABI number does not move
    assert f"#define DRIL_SAC_PENDING_CAPACITY {capi.SAC_PENDING_CAPACITY}\n" in header and capi.SAC_PENDING_CAPACITY >= 4096


def test_prototypes_and_struct_match_a_c_compile_of_the_header(pkg, tmp_path):
    capi = pkg._capi
    S = "struct dril_sac_ext_device_info"                                            # a tag only: the verb has the same name
    uses = """
    int32_t (*f1)(dril_sac_handle*, const float*, int32_t, const float*, float*, float*, void*) = dril_sac_ext_act_device;
    int32_t (*f2)(dril_sac_handle*, const float*, const uint8_t*, const uint8_t*, const float*, const float*, void*) = dril_sac_ext_push_device;
    int32_t (*f3)(dril_sac_handle*, const float*, int64_t, int32_t, const float*, float*, float*, void*) = dril_sac_predict_actions_device;
    int32_t (*f4)(dril_sac_handle*, int32_t) = dril_sac_update_enqueue;
    int32_t (*f5)(dril_sac_handle*, dril_sac_stats*, int64_t, int64_t*) = dril_sac_flush;
    int32_t (*f6)(dril_sac_handle*, const float*, const float*) = dril_sac_ext_set_action_bounds;
    int32_t (*f7)(const dril_sac_handle*, struct dril_sac_ext_device_info*) = dril_sac_ext_device_info;
    if (!f1 || !f2 || !f3 || !f4 || !f5 || !f6 || !f7) return 1;
    """
    protos = tmp_path / "protos.c"
    protos.write_text('#include "dril_sac.h"\nint use(void){' + uses + "return 0;}")
    subprocess.run(["gcc", "-Wall", "-Werror", "-Wno-unused-variable", "-I", str(ROOT / "include"), "-c", str(protos), "-o", str(tmp_path / "protos.o")], check=True)
    body = f'printf("%zu", sizeof({S}));' + "".join(f'printf(" %zu", offsetof({S}, {f}));' for f in FIELDS) + 'printf(" %d\\n", DRIL_SAC_PENDING_CAPACITY);'
    src = tmp_path / "layout.c"; exe = tmp_path / "layout"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dril_sac.h"\nint main(){' + body + "return 0;}")
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    want = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    K = capi.DrilSacExtDeviceInfo
    assert [C.sizeof(K)] + [getattr(K, f).offset for f in FIELDS] + [capi.SAC_PENDING_CAPACITY] == want
    assert tuple(n for n, _ in K._fields_) == FIELDS
    lib = capi.load_library()
    P = C.c_void_p
    for name in VERBS:
        assert hasattr(lib, name) and name in capi.EXPORTED_SYMBOLS
    assert lib.dril_sac_ext_act_device.argtypes == [P, P, C.c_int32, P, P, P, P] and lib.dril_sac_ext_push_device.argtypes == [P] * 7
    assert lib.dril_sac_predict_actions_device.argtypes == [P, P, C.c_int64, C.c_int32, P, P, P, P]
    assert lib.dril_sac_ext_device_info.argtypes == [P, C.POINTER(K)]


def test_random_action_formula_stays_inside_the_box():
    """low + u * (high - low) in float32, each operation rounded on its own (what the device computes with __fadd_rn / __fmul_rn / __fsub_rn): inside [low, high] for
    u = 0 and the largest float32 below 1, for the Boxes of the GPU tests and a few with awkward magnitudes"""
    boxes = [((-2.0,), (2.0,)), ((-1.0, -0.5, 0.25), (1.0, 0.5, 2.0)), ((-1e-3, 1e6, -3.0000002), (1e-3, 1e6 + 1, 7.1))]
    for lo, hi in boxes:
        lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
        for u in (np.float32(0), np.nextafter(np.float32(1), np.float32(0)), np.float32(0.5)):
            a = lo + u * (hi - lo)
            assert a.dtype == np.float32 and (a >= lo).all() and (a <= hi).all(), (lo, hi, u, a)
        assert np.array_equal(lo + np.float32(0) * (hi - lo), lo)


def test_null_handle_returns_before_any_gpu_work(pkg):
    capi = pkg._capi
    lib = capi.load_library()
    info = capi.DrilSacExtDeviceInfo(); info.host_syncs = 77
    NI = capi.ERR_NOT_INITIALISED
    assert lib.dril_sac_ext_act_device(None, None, 0, None, None, None, None) == NI
    assert lib.dril_sac_ext_push_device(None, None, None, None, None, None, None) == NI
    assert lib.dril_sac_predict_actions_device(None, None, 1, 0, None, None, None, None) == NI
    assert lib.dril_sac_update_enqueue(None, 1) == NI
    assert lib.dril_sac_flush(None, None, 0, None) == NI
    assert lib.dril_sac_ext_set_action_bounds(None, None, None) == NI
    assert lib.dril_sac_ext_device_info(None, C.byref(info)) == NI and info.host_syncs == 77


class _Fake:
    """carries a __cuda_array_interface__ and no memory: the checks must refuse it before any pointer is used"""

    def __init__(self, shape, typestr, strides=None, ptr=0x7f0000001000):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (ptr, False), "version": 3, "strides": strides}


class _NoLib:
    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name}) before the arguments were checked")


def _bare_handle(pkg, E=6, D=3, A=2):
    h = object.__new__(pkg.SacHandle)                                                # no dril_sac_create: no GPU here
    h.lib, h.prefix, h._h, h.E, h.D, h.A = _NoLib(), "dril_sac_", C.c_void_p(), E, D, A
    return h


def test_argument_checks_raise_before_the_library_is_called(pkg):
    h = _bare_handle(pkg)
    E, D, A = h.E, h.D, h.A
    f4 = lambda *shape, **kw: _Fake(shape, "<f4", **kw)
    u1 = lambda *shape: _Fake(shape, "|u1")
    cases = [
        (lambda: h.ext_act_device(_Fake((E, D), "<f8")), "obs", "dtype"),
        (lambda: h.ext_act_device(f4(D, E)), "obs", "(n_envs, dim)"),
        (lambda: h.ext_act_device(f4(E, D, strides=(4, 4 * E))), "obs", "C-contiguous"),
        (lambda: h.ext_act_device(f4(E, D), noise=f4(E, A + 1)), "noise", "shape"),
        (lambda: h.ext_act_device(f4(E, D), stored_actions=_Fake((E, A), "<i4")), "stored_actions", "dtype"),
        (lambda: h.ext_act_device(f4(E, D), env_actions=f4(E)), "env_actions", "shape"),
        (lambda: h.ext_act_device(np.zeros((E, D), np.float32)), "obs", "device array"),
        (lambda: h.ext_act_device(None), "obs", "None"),
        (lambda: h.ext_push_device(_Fake((E,), "<f8"), u1(E), u1(E), f4(E, D)), "rewards", "dtype"),
        (lambda: h.ext_push_device(f4(E), _Fake((E,), "<i4"), u1(E), f4(E, D)), "terminated", "dtype"),
        (lambda: h.ext_push_device(f4(E), u1(E), u1(E + 1), f4(E, D)), "truncated", "shape"),
        (lambda: h.ext_push_device(f4(E), u1(E), u1(E), None), "next_obs", "None"),
        (lambda: h.ext_push_device(f4(E), u1(E), u1(E), f4(E, D), f4(D, E)), "terminal_obs", "(n_envs, dim)"),
        (lambda: h.predict_actions_device(f4(5, D + 2), env_actions=f4(5, A)), "obs", "shape"),
        (lambda: h.predict_actions_device(f4(5, D), env_actions=f4(4, A)), "env_actions", "shape"),
        (lambda: h.predict_actions_device(f4(5, D)), "raw_actions", "at least one"),
        (lambda: h.ext_set_action_bounds(np.zeros(A + 1), np.ones(A + 1)), "low", "action_dim"),
        (lambda: h.ext_set_action_bounds(None, np.ones(A)), "low", "None"),
    ]
    for call, arg, why in cases:
        with pytest.raises(ValueError) as e:
            call()
        assert arg in str(e.value) and why in str(e.value), (arg, why, str(e.value))


def test_well_formed_arguments_reach_the_library(pkg):
    calls = []

    class _Rec:
        def __getattr__(self, name):
            return lambda *a: calls.append((name, a)) or 0

    h = _bare_handle(pkg); h.lib = _Rec()
    E, D, A = h.E, h.D, h.A
    h.ext_act_device(_Fake((E, D), "<f4", strides=(4 * D, 4)), True, None, None, _Fake((E, A), "<f4"), stream=lambda: 0x1234)
    h.ext_push_device(_Fake((E,), "<f4"), _Fake((E,), "|b1"), _Fake((E,), "|u1"), 0x7f0000002000, None, stream=0x1234)
    h.update_enqueue(3)
    assert [c[0] for c in calls] == ["dril_sac_ext_act_device", "dril_sac_ext_push_device", "dril_sac_update_enqueue"]
    act = calls[0][1]
    assert act[1].value == 0x7f0000001000 and act[2] == 1 and act[3] is None and act[4] is None and act[5].value == 0x7f0000001000 and act[6].value == 0x1234
    push = calls[1][1]
    assert push[4].value == 0x7f0000002000 and push[5] is None and push[6].value == 0x1234 and calls[2][1][1] == 3


def test_device_array_env_serves_a_sac_handle(pkg):
    """DeviceArrayParallelEnv.action_arrays asks a handle for E, A and `discrete`: a SacHandle answers (E, A) float32, allocated once"""

    class _Env:
        n_envs = 4

        def observation_space(self):
            return pkg.Box(low=[-1.0] * 3, high=[1.0] * 3)

        def action_space(self):
            return pkg.Box(low=[-1.0, 0.0], high=[1.0, 2.0])

        def reset_(self):
            pass

        def observe(self):
            return _Fake((4, 3), "<f4")

        def act_(self, actions):
            return None

    made = []
    env = pkg.DeviceArrayParallelEnv(_Env(), empty=lambda shape, dtype: made.append((shape, np.dtype(dtype))) or _Fake(shape, np.dtype(dtype).str))
    h = _bare_handle(pkg, E=4, A=2)
    a = env.action_arrays(h, None); b = env.action_arrays(h, None)
    assert made == [((4, 2), np.dtype(np.float32))] * 2 and a[0] is b[0] and a[1] is b[1]
    layer = pkg.SACLayer(env.observation_space(), env.action_space(), hidden_dims=(32, 32))
    with pytest.raises(NotImplementedError, match="one \\(low, high\\) pair"):       # the config alone carries one pair ...
        pkg.make_sac_config(env, 4, pkg.SAC(), layer)
    c = pkg.make_sac_config(env, 4, pkg.SAC(), layer, per_dim_bounds=True)           # ... the Box per dimension follows through dril_sac_ext_set_action_bounds
    assert (c.ext_action_low, c.ext_action_high, c.ext_obs_dim, c.ext_action_dim) == (-1.0, 2.0, 3, 2)
    with pytest.raises(NotImplementedError, match="normalize"):
        pkg.sac_train_(None, env, pkg.SAC(), 8, normalize=dict())
