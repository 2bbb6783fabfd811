"""The case table of the strided contraction (dril_gemm.hip), its float64 reference and the numpy emulation of the three-piece bf16 operand split
(test infrastructure of tests/test_gemm_plan.py and tests/test_gpu_gemm.py; the driver is tests/gemm_check.hip).

A case is one launch_gemm / launch_gemm_pair / launch_gemm_multi call.  Its row names the kernel it must land on (`target`, a name of dril_gemm.h
DRIL_GEMM_TARGETS); tests/test_gemm_plan.py holds every row to that through the library's own gemm_select, without a GPU.  Shapes are the smallest at which the
path can still go wrong: ragged m / n / k, more than one tile, the thresholds between kernels (K = 64, 2048 tiles, 512 blocks for two m-tiles per wave).

Every case runs in two modes:
  exact  : operands and bias are multiples of 1/8 in [-1, 1], alpha 1 or 0.5, epilogue NONE / RELU / MASK_RELU (a case's other epilogues map onto those three):
           every product and partial sum is exact in f32, and in the bf16 split too (a 4-bit mantissa sits in the first piece, the other two are zero), so EVERY
           kernel must equal the float64 reference bit for bit, whatever its summation order;
  normal : standard-normal operands, the case's own epilogue, against the error bound of `tolerance`.
Buffer images: operands have padded leading dimensions and >= 4 KB behind them, all of it NaN (a result that depends on memory outside the logical operand turns
NaN); C / zout images are sentinels, including the padding between columns and a guard before and after.
"""
from __future__ import annotations

import hashlib
import re
import subprocess
from dataclasses import dataclass, field, replace
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "dril.jl_amd" / "csrc"
SENTINEL = np.float32(-7777.5)                      # tests/gemm_check.hip kSentinel
SLACK = 1024                                        # floats of NaN behind every operand image (4 KB)
GUARD = 64                                          # sentinel floats before and after the logical C

EPI = {"NONE": 0, "RELU": 1, "TANH": 2, "MASK_RELU": 3, "MASK_TANH": 4, "SIGMOID": 5, "ELU": 6, "LEAKY": 7, "SOFTPLUS": 8, "MASK_SIGMOID": 9, "MASK_ELU": 10,
       "MASK_LEAKY": 11, "MASK_SOFTPLUS": 12, "GELU": 13, "SWISH": 14, "MASK_GELU": 15, "MASK_SWISH": 16}          # dril_gemm.h
MASKS = {n for n in EPI if n.startswith("MASK_")}
TARGETS = ["direct_splitk", "direct_tiles", "lds_00", "lds_01", "lds_10", "lds_11", "big_am_bk", "big_ak_bk", "big_am_bn", "big_ak_bn"] + \
          [f"split_{a}_{b}_mb{m}" for m in (1, 2) for b in ("bk", "bn") for a in ("am", "ak")]
SIX_EPI = [("NONE", False), ("RELU", False), ("TANH", False), ("MASK_TANH", False), ("GELU", True), ("MASK_SWISH", False)]


def r4(x):
    return (x + 3) // 4 * 4


@dataclass(frozen=True)
class Con:
    """one contraction C[z](M x N) = epi(alpha A[z](M x K) B[z / zdivB](K x N) + bias[z](M)); a: A is "m"- or "k"-contiguous, b: B is "k"- or "n"-contiguous"""
    M: int
    N: int
    K: int
    Z: int = 1
    a: str = "m"
    b: str = "k"
    ones: bool = False            # B's last column is the synthetic ones column (not in memory)
    zdivB: int = 1
    bias: bool = True
    epi: str = "NONE"
    zout: bool = False
    alpha: float = 1.0            # exact mode (1 or 0.5)
    alpha_normal: float = None    # normal mode; default = alpha
    a_off: int = 0                # A starts this many floats into its (16-byte aligned) image
    ldb_odd: bool = False         # n-contiguous B with a leading dimension that is no multiple of 4 (vecBn = 0)

    def layout(self):
        M, N, K, Z = self.M, self.N, self.K, self.Z
        nr = N - (1 if self.ones else 0)
        ldk = r4(K) + 4 if K % 4 == 0 else K + 5
        L = {"n_real": nr}
        if self.a == "m":
            ld = r4(M) + 4
            L.update(sAm=1, sAk=ld, extA=K * ld)
        else:
            L.update(sAm=ldk, sAk=1, extA=M * ldk)
        if self.b == "k":
            L.update(sBn=ldk, sBk=1, extB=nr * ldk)
        else:
            ld = r4(nr) + (5 if self.ldb_odd else 4)
            L.update(sBk=ld, sBn=1, extB=K * ld)
        L["zA"], L["zB"] = r4(L["extA"]) + 8, r4(L["extB"]) + 8
        L["ZB"] = (Z - 1) // self.zdivB + 1
        L["sCm"], L["sCn"] = 1, M + 3
        L["zC"] = N * L["sCn"] + 5
        L["totalC"] = GUARD + Z * L["zC"] + GUARD
        return L


@dataclass(frozen=True)
class Case:
    name: str
    target: str                   # "lds_01", "pair:lds_01+direct_splitk", ...
    cons: tuple
    kind: int = 0                 # 0 launch_gemm, 1 launch_gemm_pair, 2 launch_gemm_multi
    allow_split: int = 0


def _single(name, target, con, allow_split=0):
    return Case(name, target, (con,), 0, allow_split)


def _table():
    T = []
    big = dict(M=40, N=8200, Z=4)                    # tm 2 x tn 257 x Z 4 = 2056 tiles; tn = 257 leaves one live wave in the last workgroup
    # ---- direct split-K: fewer than 2048 tiles and K < 64, or an operand that fits no vector pattern
    T += [_single("d_1x1x1", "direct_splitk", Con(1, 1, 1)),
          _single("d_33x31x7", "direct_splitk", Con(33, 31, 7, a="m", b="k")),
          _single("d_40x70x63", "direct_splitk", Con(40, 70, 63, Z=2, a="k", b="n")),
          _single("d_5x37x520_aoff", "direct_splitk", Con(5, 37, 520, a="k", b="k", a_off=1)),      # 65 chunks over 8 waves: 9 per wave, second depth iteration
          _single("d_6x12x40_ones", "direct_splitk", Con(6, 12, 40, a="m", b="n", ones=True))]
    for e in EPI:                                                                                    # all 17 epilogues
        T.append(_single(f"d_epi_{e.lower()}", "direct_splitk", Con(34, 33, 10, Z=2, a="m", b="k", epi=e, zout=e in ("GELU", "SWISH"), alpha_normal=0.25)))
    # ---- LDS-staged split-K, the four access-pattern pairs
    T += [_single("l00_1x1x64", "lds_00", Con(1, 1, 64, a="k", b="k")),
          _single("l00_31x33x260", "lds_00", Con(31, 33, 260, a="k", b="k")),
          _single("l00_65x100x516_z3", "lds_00", Con(65, 100, 516, Z=3, a="k", b="k")),
          _single("l01_33x65x64", "lds_01", Con(33, 65, 64, a="k", b="n")),
          _single("l01_100x31x260_zdiv2", "lds_01", Con(100, 31, 260, Z=4, zdivB=2, a="k", b="n")),
          _single("l01_65x1x516", "lds_01", Con(65, 1, 516, a="k", b="n")),
          _single("l10_31x100x64", "lds_10", Con(31, 100, 64, a="m", b="k")),
          _single("l10_1x33x260", "lds_10", Con(1, 33, 260, a="m", b="k")),
          _single("l10_33x31x516_alpha", "lds_10", Con(33, 31, 516, a="m", b="k", alpha=0.5)),
          _single("l11_65x33x67", "lds_11", Con(65, 33, 67, a="m", b="n")),
          _single("l11_100x65x257_z3", "lds_11", Con(100, 65, 257, Z=3, zdivB=1, a="m", b="n")),
          _single("l11_1x31x260", "lds_11", Con(1, 31, 260, a="m", b="n"))]
    for N in (33, 34, 35, 36):                                                                       # the ones row alone in a tile / at each position of a float4 group
        a = "m" if N % 2 else "k"
        T.append(_single(f"l{'1' if a == 'm' else '0'}1_ones_n{N}", "lds_11" if a == "m" else "lds_01", Con(40, N, 67 if a == "m" else 64, Z=2, a=a, b="n", ones=True)))
    for e, z in SIX_EPI:
        T.append(_single(f"l10_epi_{e.lower()}", "lds_10", Con(33, 40, 68, Z=2, a="m", b="k", epi=e, zout=z, alpha_normal=0.125)))
    # ---- tile-parallel direct: >= 2048 tiles, K < 32 or B fits no vector pattern
    T += [_single("t_40x8200x4", "direct_tiles", Con(K=4, a="m", b="k", **big)),
          _single("t_40x8200x70_bk", "direct_tiles", Con(K=70, a="m", b="k", **big))]
    # ---- big (LDS-tiled f32 MFMA), four layouts
    T += [_single("b_am_bk_k32", "big_am_bk", Con(K=32, a="m", b="k", **big)),
          _single("b_ak_bk_k36", "big_ak_bk", Con(K=36, a="k", b="k", **big)),
          _single("b_am_bk_k100", "big_am_bk", Con(K=100, a="m", b="k", zdivB=2, **big)),
          _single("b_am_bn_k33", "big_am_bn", Con(K=33, a="m", b="n", **big)),
          _single("b_ak_bn_k33", "big_ak_bn", Con(K=33, a="k", b="n", zdivB=4, **big)),
          _single("b_am_bn_ones_z137", "big_am_bn", Con(65, 130, 40, Z=137, a="m", b="n", ones=True)),          # n_real = 129 straddles a float4
          _single("b_ak_bn_ones_z137_ldodd", "big_ak_bn", Con(65, 130, 40, Z=137, a="k", b="n", ones=True, ldb_odd=True))]
    for e, z in SIX_EPI:
        T.append(_single(f"b_epi_{e.lower()}", "big_am_bk", Con(33, 70, 36, Z=342, a="m", b="k", epi=e, zout=z, alpha_normal=0.125)))
    # ---- split (bf16 three-piece operand split), eight forms
    T += [_single("s_am_bk_k64", "split_am_bk_mb1", Con(K=64, a="m", b="k", **big), 1),
          _single("s_ak_bk_k72", "split_ak_bk_mb1", Con(K=72, a="k", b="k", **big), 1),
          _single("s_am_bk_k200", "split_am_bk_mb1", Con(K=200, a="m", b="k", zdivB=2, **big), 1),
          _single("s_am_bn_k77", "split_am_bn_mb1", Con(K=77, a="m", b="n", **big), 1),
          _single("s_ak_bn_k77_ones", "split_ak_bn_mb1", Con(K=77, a="k", b="n", ones=True, zdivB=4, **big), 1),
          _single("s2_am_bk_m70", "split_am_bk_mb2", Con(70, 16400, 72, Z=4, zdivB=4, a="m", b="k"), 1),        # the second m-tile of the second block lies outside M
          _single("s2_ak_bk_m96", "split_ak_bk_mb2", Con(96, 16400, 72, Z=4, zdivB=2, a="k", b="k"), 1),
          _single("s2_am_bn_m96", "split_am_bn_mb2", Con(96, 16400, 72, Z=4, zdivB=4, a="m", b="n"), 1),
          _single("s2_ak_bn_m70", "split_ak_bn_mb2", Con(70, 16400, 72, Z=4, zdivB=2, a="k", b="n"), 1)]
    for e, z in SIX_EPI:
        T.append(_single(f"s_epi_{e.lower()}", "split_am_bk_mb1", Con(33, 70, 72, Z=342, a="m", b="k", epi=e, zout=z, alpha_normal=0.125), 1))
    # ---- pair: [dW | db] on the LDS body beside a short masked contraction on the direct body; different batch counts and tile grids
    dw = Con(40, 65, 256, Z=2, a="k", b="n", ones=True, bias=False)
    dz = Con(64, 256, 6, Z=3, a="m", b="k", epi="MASK_TANH", alpha_normal=0.25)
    T += [Case("p_dw_dz", "pair:lds_01+direct_splitk", (dw, dz), 1),
          Case("p_dz_dw", "pair:direct_splitk+lds_01", (dz, dw), 1)]
    # ---- multi: 1, 3, 4 contractions of differing shapes
    m0 = Con(33, 40, 68, Z=2, a="m", b="k", epi="RELU")
    m2 = Con(31, 33, 67, Z=3, a="m", b="n", epi="MASK_RELU")
    m3 = Con(5, 37, 520, a="k", b="k", a_off=1)
    T += [Case("m_n1", "multi:lds_10", (m0,), 2),
          Case("m_n3", "multi:lds_01+direct_splitk+lds_11", (dw, dz, m2), 2),
          Case("m_n4", "multi:lds_11+lds_10+direct_splitk+lds_01", (m2, m0, m3, dw), 2)]
    return T


CASES = _table()
SPLIT_CASES = [c for c in CASES if c.target.startswith("split_")]
MODES = ("exact", "normal")


def big_twin(case):
    """the same operands through the exact-f32 big kernel (allow_split = 0): the yardstick of the split criterion"""
    return replace(case, name=case.name + "_f32", target=case.target.replace("split", "big")[:-4], allow_split=0)


def run_name(case, mode):
    return f"{case.name}.{mode}"


def data_key(case):
    """operands are a function of the case's shapes, not of its kernel: a split case and its f32 twin read the same images"""
    return case.name[:-4] if case.name.endswith("_f32") else case.name


def exact_epi(epi):
    return "NONE" if epi == "NONE" else "MASK_RELU" if epi in MASKS else "RELU"


def mode_epi_alpha(con, mode):
    if mode == "exact":
        return exact_epi(con.epi), con.alpha
    return con.epi, con.alpha if con.alpha_normal is None else con.alpha_normal


# =====================================================================================================================
# activations: the NNlib formulas that include/device/dril_activations.h cites, generic over the float type of x
# =====================================================================================================================
def _sigmoid(x):
    one = x.dtype.type(1)
    return one / (one + np.exp(-x))


def _gelu_u(x):
    t = x.dtype.type
    return t(np.sqrt(2.0 / np.pi)) * (x + t(0.044715) * x * x * x)


def epilogue(epi, v, y):
    """v = alpha A.B + bias, y = aux (the activation's output, or for gelu / swish the pre-activation); evaluated in v's dtype"""
    t = v.dtype.type
    if epi == "NONE":
        return v
    if epi == "RELU":
        return np.maximum(v, t(0))
    if epi == "TANH":
        return np.tanh(v)
    if epi == "SIGMOID":
        return _sigmoid(v)
    if epi == "ELU":
        return np.where(v > 0, v, np.expm1(np.minimum(v, t(0))))
    if epi == "LEAKY":
        return np.where(v > 0, v, t(0.01) * v)
    if epi == "SOFTPLUS":
        return np.maximum(v, t(0)) + np.log1p(np.exp(-np.abs(v)))
    if epi == "GELU":
        return t(0.5) * v * (t(1) + np.tanh(_gelu_u(v)))
    if epi == "SWISH":
        return v * _sigmoid(v)
    if epi == "MASK_RELU":
        return np.where(y > 0, v, t(0))
    if epi == "MASK_TANH":
        return v * (t(1) - y * y)
    if epi == "MASK_SIGMOID":
        return v * (y * (t(1) - y))
    if epi == "MASK_ELU":
        return v * np.where(y > 0, t(1), y + t(1))
    if epi == "MASK_LEAKY":
        return v * np.where(y > 0, t(1), t(0.01))
    if epi == "MASK_SOFTPLUS":
        return v * -np.expm1(-y)
    if epi == "MASK_GELU":
        th = np.tanh(_gelu_u(y))
        return v * (t(0.5) * (t(1) + th) + t(0.5) * y * (t(1) - th * th) * t(np.sqrt(2.0 / np.pi)) * (t(1) + t(3 * 0.044715) * y * y))
    if epi == "MASK_SWISH":
        s = _sigmoid(y)
        return v * (s * (t(1) + y * (t(1) - s)))
    raise ValueError(epi)


MAX_SLOPE = 1.13                 # the largest |d epi / d v| over the 17 epilogues: gelu' peaks at 1.129 (the mask epilogues multiply v by that same derivative)
ACT_MARGIN = 4.0                 # composite device formulas compound three to four libm roundings


# =====================================================================================================================
# operands, buffer images, reference
# =====================================================================================================================
def _rng(case, i, mode):
    h = hashlib.sha256(f"{data_key(case)}/{i}/{mode}".encode()).digest()
    return np.random.default_rng(int.from_bytes(h[:8], "little"))


def _draw(rng, shape, mode):
    if mode == "exact":
        return (rng.integers(-8, 9, size=shape) / 8.0).astype(np.float32)
    return rng.standard_normal(shape, dtype=np.float32)


def operands(case, i, mode):
    """logical operands of contraction i: A (Z, M, K), B (ZB, K, n_real), bias (Z, M) or None, aux (Z, M, N) or None — float32"""
    con, rng = case.cons[i], _rng(case, i, mode)
    L = con.layout()
    epi, _ = mode_epi_alpha(con, mode)
    A = _draw(rng, (con.Z, con.M, con.K), mode)
    B = _draw(rng, (L["ZB"], con.K, L["n_real"]), mode)
    bias = _draw(rng, (con.Z, con.M), mode) if con.bias else None
    aux = None
    if epi in MASKS:
        aux = _draw(rng, (con.Z, con.M, con.N), mode)
        if mode == "normal" and epi not in ("MASK_GELU", "MASK_SWISH", "MASK_RELU"):               # the activation's OUTPUT: in its range
            aux = epilogue(epi[5:], aux, None).astype(np.float32)
    return A, B, bias, aux


def _image(total, off, zstride, s_row, s_col, x):
    """x (Z, R, C) laid out at off + z zstride + r s_row + c s_col in a NaN image"""
    img = np.full(total, np.nan, np.float32)
    Z, R, C = x.shape
    idx = off + (np.arange(Z) * zstride)[:, None, None] + (np.arange(R) * s_row)[None, :, None] + (np.arange(C) * s_col)[None, None, :]
    img[idx] = x
    return img


def write_images(case, mode, data_dir):
    """the operand images of one (case, mode) under data_dir (shared by a split case and its f32 twin)"""
    data_dir = Path(data_dir)
    for i, con in enumerate(case.cons):
        stem = f"{data_key(case)}.{mode}.{i}"
        if (data_dir / f"{stem}.A.bin").exists():
            continue
        L = con.layout()
        A, B, bias, aux = operands(case, i, mode)
        _image(con.a_off + con.Z * L["zA"] + SLACK, con.a_off, L["zA"], L["sAm"], L["sAk"], A).tofile(data_dir / f"{stem}.A.bin")
        _image(L["ZB"] * L["zB"] + SLACK, 0, L["zB"], L["sBk"], L["sBn"], B).tofile(data_dir / f"{stem}.B.bin")
        if bias is not None:
            np.concatenate([bias.ravel(), np.full(SLACK, np.nan, np.float32)]).tofile(data_dir / f"{stem}.bias.bin")
        if aux is not None:
            _image(L["totalC"], GUARD, L["zC"], L["sCm"], L["sCn"], aux).tofile(data_dir / f"{stem}.aux.bin")


def case_lines(case, mode):
    out = [f"case {run_name(case, mode)} {case.kind} {len(case.cons)} {case.allow_split}"]
    for i, con in enumerate(case.cons):
        L = con.layout()
        epi, alpha = mode_epi_alpha(con, mode)
        stem = f"{data_key(case)}.{mode}.{i}"
        out.append(" ".join(str(x) for x in (
            "g", con.M, con.N, con.K, con.Z, L["sAm"], L["sAk"], L["sBk"], L["sBn"], L["sCm"], L["sCn"], L["zA"], L["zB"], L["zC"], con.M, L["zC"], con.zdivB,
            int(con.ones), EPI[epi], repr(float(alpha)), int(con.zout), f"{stem}.A.bin", con.a_off, f"{stem}.B.bin", 0,
            f"{stem}.bias.bin" if con.bias else "-", f"{stem}.aux.bin" if epi in MASKS else "-", L["totalC"], GUARD)))
    return out


def write_case_file(path, runs):
    """runs: (case, mode) pairs"""
    Path(path).write_text("\n".join(line for case, mode in runs for line in case_lines(case, mode)) + "\n")


def logical(con, img):
    """(the logical (Z, M, N) view of a C / zout image, a mask of the image's elements outside it)"""
    L = con.layout()
    idx = GUARD + (np.arange(con.Z) * L["zC"])[:, None, None] + (np.arange(con.M) * L["sCm"])[None, :, None] + (np.arange(con.N) * L["sCn"])[None, None, :]
    outside = np.ones(img.shape, bool)
    outside[idx] = False
    return img[idx], outside


def reference(case, i, mode):
    """float64: (C, pre-activation, bound) of contraction i.  bound = (K + 16) 2^-24 (|alpha| sum_k |a_k b_k| + |bias|): the worst case of K fused
    accumulations in any order, the 8-wave reduction, alpha and bias"""
    con = case.cons[i]
    epi, alpha = mode_epi_alpha(con, mode)
    A, B, bias, aux = (None if x is None else x.astype(np.float64) for x in operands(case, i, mode))
    if con.ones:
        B = np.concatenate([B, np.ones((B.shape[0], con.K, 1))], axis=2)
    Bz = B[np.arange(con.Z) // con.zdivB]
    b = bias[:, :, None] if bias is not None else 0.0
    pre = alpha * np.matmul(A, Bz) + b
    bound = (con.K + 16) * 2.0 ** -24 * (abs(alpha) * np.matmul(np.abs(A), np.abs(Bz)) + np.abs(b))
    return epilogue(epi, pre, aux), pre, bound


def tolerance(con, mode, pre, aux32, bound):
    """per-element tolerance of C in normal mode.  NONE: the pre-activation bound.  Any other epilogue: the bound times the largest slope of the 17 epilogues, plus
    ACT_MARGIN times the rounding of the activation's own evaluation, MEASURED ON THE REFERENCE: the largest distance between the numpy-float32 and the float64
    evaluation of the same formula over this case's own pre-activations"""
    epi, _ = mode_epi_alpha(con, mode)
    if epi == "NONE":
        return bound, 0.0
    y64 = None if aux32 is None else aux32.astype(np.float64)
    spread = float(np.max(np.abs(epilogue(epi, pre.astype(np.float32), aux32).astype(np.float64) - epilogue(epi, pre, y64))))
    return MAX_SLOPE * bound + ACT_MARGIN * spread, spread


# =====================================================================================================================
# numpy emulation of the operand split (dril_device.h split3_pair, sac_gemm_split_kernel) and of the f32 MFMA chain
# =====================================================================================================================
def bf16_round(x, rounding="nearest"):
    """f32 -> the nearest (ties to even; v_cvt_pk_bf16_f32, what split3_pair uses) or the truncated (upper 16 bits) bf16 value, as f32"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    if rounding == "nearest":
        u = u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))
    return (u & np.uint32(0xFFFF0000)).view(np.float32)


def split3(x, rounding="nearest"):
    """x = hi + mid + lo: a bf16 piece, the exact f32 remainder, twice"""
    x = np.asarray(x, np.float32)
    hi = bf16_round(x, rounding)
    r = x - hi
    mid = bf16_round(r, rounding)
    q = r - mid
    lo = bf16_round(q, rounding)
    return hi, mid, lo


def emulate_split(A, B, products=6, rounding="nearest"):
    """A (M, K) . B (K, N) as sac_gemm_split_kernel contracts it: per k16 step the piece products in the kernel's order (small terms first), each one MFMA whose 16
    products are exact and whose sum is rounded into the f32 accumulator.  products = 4: without Al.Bh and Ah.Bl (the DRIL_DEBUG_DROP_LO negative control)"""
    Ah, Am, Al = (p.astype(np.float64) for p in split3(A, rounding))
    Bh, Bm, Bl = (p.astype(np.float64) for p in split3(B, rounding))
    order = [(Al, Bh), (Ah, Bl), (Am, Bm), (Am, Bh), (Ah, Bm), (Ah, Bh)][6 - products:]
    acc = np.zeros((A.shape[0], B.shape[1]), np.float32)
    for k in range(0, A.shape[1], 16):
        for a, b in order:
            acc = (acc.astype(np.float64) + a[:, k:k + 16] @ b[k:k + 16]).astype(np.float32)
    return acc


def emulate_f32(A, B):
    """the v_mfma_f32_32x32x2_f32 chain of the big kernel: one fused multiply-add per k into an f32 accumulator"""
    A64, B64 = A.astype(np.float64), B.astype(np.float64)
    acc = np.zeros((A.shape[0], B.shape[1]), np.float32)
    for k in range(A.shape[1]):
        acc = (acc.astype(np.float64) + np.outer(A64[:, k], B64[k])).astype(np.float32)
    return acc


def rms(x):
    return float(np.sqrt(np.mean(np.square(x, dtype=np.float64))))


# =====================================================================================================================
# the driver
# =====================================================================================================================
def driver_flags():
    """the library's own compile flags (csrc/Makefile CXXFLAGS), so that the driver's kernels are the product's"""
    m = re.search(r"^CXXFLAGS \?= (.*)$", (CSRC / "Makefile").read_text(), re.M)
    return m.group(1).replace("$(ARCH)", "gfx950").split()


def build_driver(droplo=False):
    """compiles tests/gemm_check.hip (about 25 s) into build/gemm_check/, once per content of its sources and flags"""
    src = ROOT / "tests" / "gemm_check.hip"
    deps = [src, CSRC / "dril_gemm.hip", CSRC / "dril_gemm.h", CSRC / "dril_device.h", ROOT / "include" / "device" / "dril_activations.h"]
    flags = driver_flags() + (["-DDRIL_DEBUG_DROP_LO"] if droplo else [])
    h = hashlib.sha256(" ".join(flags).encode())
    for d in deps:
        h.update(d.read_bytes())
    out = ROOT / "build" / "gemm_check" / f"gemm_check{'_droplo' if droplo else ''}-{h.hexdigest()[:16]}"
    if not out.exists():
        out.parent.mkdir(parents=True, exist_ok=True)
        tmp = out.with_suffix(".tmp")
        subprocess.run(["/opt/rocm/bin/hipcc", *flags, "-I", str(CSRC), "-o", str(tmp), str(src)], check=True)
        tmp.replace(out)
    return out
