"""CPU: the device-array verbs of DRIL_ENV_EXTERNAL (dril_ext_act_device / _record_device / _finish_device, dril_predict_actions_device,
dril_ext_set_action_bounds, dril_ext_device_info; docs/external_envs.md section 10), without a GPU.

  * the prototypes and the info struct: a C compile against include/dril_hip.h, compared with the ctypes mirror;
  * the Python argument checks raise a ValueError that names the argument BEFORE the library is called (fake objects with __cuda_array_interface__);
  * DeviceArrayParallelEnv refuses an env whose act_ returns three values;
  * the Julia shim's static check still passes."""
import ctypes as C
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
VERBS = ("dril_ext_act_device", "dril_ext_record_device", "dril_ext_finish_device", "dril_predict_actions_device", "dril_ext_set_action_bounds", "dril_ext_device_info")
FIELDS = ("steps_device", "steps_host", "host_syncs", "per_dim_bounds", "launches", "reserved")


def test_prototypes_and_struct_match_a_c_compile_of_the_header(pkg, tmp_path):
    capi = pkg._capi
    S = "struct dril_ext_device_info"                                                 # a tag only: the verb has the same name
    body = f'printf("%zu", sizeof({S}));' + "".join(f'printf(" %zu", offsetof({S}, {f}));' for f in FIELDS) + 'printf("\\n");'
    # the prototypes, used as the issue states them: assigning to typed function pointers fails to compile on any mismatch (-Werror)
    uses = """
    int32_t (*f1)(dril_handle*, const float*, void*, void*, void*) = dril_ext_act_device;
    int32_t (*f2)(dril_handle*, const float*, const uint8_t*, const uint8_t*, const float*, void*) = dril_ext_record_device;
    int32_t (*f3)(dril_handle*, const float*, void*) = dril_ext_finish_device;
    int32_t (*f4)(dril_handle*, const float*, int64_t, int32_t, void*, void*, void*) = dril_predict_actions_device;
    int32_t (*f5)(dril_handle*, const float*, const float*) = dril_ext_set_action_bounds;
    int32_t (*f6)(const dril_handle*, struct dril_ext_device_info*) = dril_ext_device_info;
    if (!f1 || !f2 || !f3 || !f4 || !f5 || !f6) return 1;
    """
    protos = tmp_path / "protos.c"
    protos.write_text('#include "dril_hip.h"\nint use(void){' + uses + "return 0;}")
    subprocess.run(["gcc", "-Wall", "-Werror", "-Wno-unused-variable", "-I", str(ROOT / "include"), "-c", str(protos), "-o", str(tmp_path / "protos.o")], check=True)
    src = tmp_path / "layout.c"; exe = tmp_path / "layout"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dril_hip.h"\nint main(){' + body + "return 0;}")
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    want = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    K = capi.DrilExtDeviceInfo
    assert [C.sizeof(K)] + [getattr(K, f).offset for f in FIELDS] == want
    assert tuple(n for n, _ in K._fields_) == FIELDS
    header = (ROOT / "include" / "dril_hip.h").read_text()
    assert "#define DRIL_ABI_VERSION 2u" in header and capi.ABI_VERSION == 2         # dril_config and the ABI number do not move
    lib = capi.load_library()
    P = C.c_void_p
    for name in VERBS:
        assert hasattr(lib, name) and name in capi.EXPORTED_SYMBOLS
    assert lib.dril_ext_act_device.argtypes == [P] * 5 and lib.dril_ext_record_device.argtypes == [P] * 6 and lib.dril_ext_finish_device.argtypes == [P] * 3
    assert lib.dril_predict_actions_device.argtypes == [P, P, C.c_int64, C.c_int32, P, P, P]
    assert lib.dril_ext_device_info.argtypes == [P, C.POINTER(K)]


def test_null_handle_returns_before_any_gpu_work(pkg):
    capi = pkg._capi
    lib = capi.load_library()
    info = capi.DrilExtDeviceInfo(); info.host_syncs = 77
    assert lib.dril_ext_act_device(None, None, None, None, None) == capi.ERR_NOT_INITIALISED
    assert lib.dril_ext_record_device(None, None, None, None, None, None) == capi.ERR_NOT_INITIALISED
    assert lib.dril_ext_finish_device(None, None, None) == capi.ERR_NOT_INITIALISED
    assert lib.dril_predict_actions_device(None, None, 1, 0, None, None, None) == capi.ERR_NOT_INITIALISED
    assert lib.dril_ext_set_action_bounds(None, None, None) == capi.ERR_NOT_INITIALISED
    assert lib.dril_ext_device_info(None, C.byref(info)) == capi.ERR_NOT_INITIALISED and info.host_syncs == 77


class _Fake:
    """carries a __cuda_array_interface__ and no memory: the checks must refuse it before any pointer is used"""

    def __init__(self, shape, typestr, strides=None, ptr=0x7f0000001000):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (ptr, False), "version": 3, "strides": strides}


class _NoLib:
    """stands where the library would be: any call through it fails the test"""

    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name}) before the arguments were checked")


def _bare_handle(pkg, E=6, D=3, A=2, discrete=False):
    h = object.__new__(pkg.Handle)                                                    # no dril_create: no GPU here
    h.lib, h._h, h.E, h.D, h.A, h.discrete, h.T = _NoLib(), C.c_void_p(), E, D, A, discrete, 2
    return h


def test_argument_checks_raise_before_the_library_is_called(pkg):
    h = _bare_handle(pkg)
    E, D, A = h.E, h.D, h.A
    f4 = lambda *shape, **kw: _Fake(shape, "<f4", **kw)
    u1 = lambda *shape: _Fake(shape, "|u1")
    cases = [
        # (call, the argument the message must name, a fragment of the reason)
        (lambda: h.ext_act_device(_Fake((E, D), "<f8")), "obs", "dtype"),                                   # a wrong dtype
        (lambda: h.ext_act_device(f4(E, D + 1)), "obs", "shape"),                                           # a wrong shape
        (lambda: h.ext_act_device(f4(D, E)), "obs", "(n_envs, dim)"),                                       # (D, E) where (E, D) is expected
        (lambda: h.ext_act_device(f4(E, D, strides=(4, 4 * E))), "obs", "C-contiguous"),                    # a transposed view
        (lambda: h.ext_act_device(f4(E, D, strides=(8 * D, 8))), "obs", "C-contiguous"),                    # every second element
        (lambda: h.ext_act_device(f4(E, D), raw_actions=_Fake((E, A), "<i4")), "raw_actions", "dtype"),
        (lambda: h.ext_act_device(f4(E, D), env_actions=f4(E)), "env_actions", "shape"),
        (lambda: h.ext_act_device(np.zeros((E, D), np.float32)), "obs", "device array"),                    # a host array
        (lambda: h.ext_act_device(None), "obs", "None"),
        (lambda: h.ext_record_device(_Fake((E,), "<f8"), u1(E), u1(E)), "rewards", "dtype"),
        (lambda: h.ext_record_device(f4(E), _Fake((E,), "<i4"), u1(E)), "terminated", "dtype"),
        (lambda: h.ext_record_device(f4(E), u1(E), u1(E + 1)), "truncated", "shape"),
        (lambda: h.ext_record_device(f4(E), u1(E), u1(E), f4(D, E)), "terminal_obs", "(n_envs, dim)"),
        (lambda: h.ext_finish_device(f4(E * D)), "last_obs", "shape"),
        (lambda: h.predict_actions_device(f4(5, D + 2), env_actions=f4(5, A)), "obs", "shape"),
        (lambda: h.predict_actions_device(f4(5, D), env_actions=f4(4, A)), "env_actions", "shape"),
        (lambda: h.predict_actions_device(f4(5, D)), "raw_actions", "at least one"),
        (lambda: h.ext_set_action_bounds(np.zeros(A + 1), np.ones(A + 1)), "low", "action_dim"),
    ]
    for call, arg, why in cases:
        with pytest.raises(ValueError) as e:
            call()
        assert arg in str(e.value) and why in str(e.value), (arg, why, str(e.value))
    hd = _bare_handle(pkg, discrete=True)
    with pytest.raises(ValueError, match="env_actions"):
        hd.ext_act_device(f4(E, D), env_actions=_Fake((E, hd.A), "<i4"))             # Discrete actions are (E,)
    with pytest.raises(ValueError, match="raw_actions"):
        hd.ext_act_device(f4(E, D), raw_actions=f4(E))                               # and int32


def test_well_formed_arguments_reach_the_library(pkg):
    """the same fakes with the right shape / dtype pass the checks: bool flags, explicit C strides, raw integer pointers, a callable stream"""
    calls = []

    class _Rec:
        def __getattr__(self, name):
            return lambda *a: calls.append((name, a)) or 0

    h = _bare_handle(pkg); h.lib = _Rec()
    E, D, A = h.E, h.D, h.A
    h.ext_act_device(_Fake((E, D), "<f4", strides=(4 * D, 4)), env_actions=_Fake((E, A), "<f4"), stream=lambda: 0x1234)
    h.ext_record_device(_Fake((E,), "<f4"), _Fake((E,), "|b1"), _Fake((E,), "|u1"), None, stream=0x1234)
    h.ext_finish_device(0x7f0000002000)
    names = [c[0] for c in calls]
    assert names == ["dril_ext_act_device", "dril_ext_record_device", "dril_ext_finish_device"]
    act = calls[0][1]
    assert act[1].value == 0x7f0000001000 and act[2] is None and act[3].value == 0x7f0000001000 and act[4].value == 0x1234
    assert calls[1][1][4] is None and calls[1][1][5].value == 0x1234
    assert calls[2][1][1].value == 0x7f0000002000 and calls[2][1][2] is None        # stream None = the null stream


class _ThreeValueEnv:
    n_envs = 4

    def __init__(self, pkg):
        self.pkg = pkg

    def observation_space(self):
        return self.pkg.Box(low=[-1.0] * 3, high=[1.0] * 3)

    def action_space(self):
        return self.pkg.Discrete(2)

    def reset_(self):
        pass

    def observe(self):
        return _Fake((4, 3), "<f4")

    def act_(self, actions):
        return _Fake((4,), "<f4"), _Fake((4,), "|u1"), _Fake((4,), "|u1")            # no terminal_obs slot


def test_device_array_env_rejects_an_act_with_three_values(pkg):
    env = pkg.DeviceArrayParallelEnv(_ThreeValueEnv(pkg))
    assert env.kind == pkg._capi.ENV_EXTERNAL and env.number_of_envs() == 4 and isinstance(env.action_space(), pkg.Discrete)
    with pytest.raises(ValueError, match="got 3 values"):
        env.act_(_Fake((4,), "<i4"))
    with pytest.raises(TypeError, match="n_envs"):
        pkg.DeviceArrayParallelEnv(object())
    with pytest.raises(ValueError, match="empty="):                                  # an array library the wrapper does not know needs the factory
        env.action_arrays(_bare_handle(pkg, E=4, discrete=True), _Fake((4, 3), "<f4"))
    made = []
    env2 = pkg.DeviceArrayParallelEnv(_ThreeValueEnv(pkg), empty=lambda shape, dtype: made.append((shape, np.dtype(dtype))) or _Fake(shape, np.dtype(dtype).str))
    hb = _bare_handle(pkg, E=4, discrete=True)
    a = env2.action_arrays(hb, None); b = env2.action_arrays(hb, None)
    assert made == [((4,), np.dtype(np.int32))] * 2 and a[0] is b[0] and a[1] is b[1]   # allocated once


def test_shim_check_still_passes():
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "check_shim.py")], capture_output=True, text=True)
    assert r.returncode == 0 and "check_shim: ok" in r.stdout, r.stdout[-2000:]
