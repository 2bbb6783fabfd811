// dril_gemm.h — the generic strided fp32-MFMA contraction shared by the SAC path (dril_sac_net.hip) and the generic
// (any obs / action / hidden width) on-policy path (dril_generic.hip).  Kernels in dril_gemm.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdlib>

namespace dril {

// C[z](M x N) = epi(alpha * A[z](M x K) . B[z](K x N) + bias[z](M)), every operand addressed by element strides
struct GemmArgs {
    const float* A; const float* B; float* C; const float* bias; const float* aux;
    float* zout;                                  // when set: the pre-activation alpha * A.B + bias goes here too (C's strides), for activations whose derivative needs it (gelu, swish)
    int M, N, K;
    int sAm, sAk, sBk, sBn, sCm, sCn;             // element strides
    long long zA, zB, zC, zBias, zAux;            // batch (blockIdx.z) strides
    int zdivB;                                    // B uses batch index z / zdivB (several nets reading one input)
    int vecA, vecB;                               // operand has unit stride along k, 16-byte aligned rows and K % 4 == 0: float4 loads
    int use_lds;                                  // the LDS-staged (coalesced-load) split-K body for this contraction (set by gemm_prepare: K >= 64)
    int ldsA, ldsB;                               // access pattern of the LDS-staged split-K shape (set by gemm_prepare): 0 k-contiguous float4, 1 row-contiguous float4, 2 element by element
    int vecBn;                                    // B has unit stride along n with 16-byte aligned rows: float4 runs along n (LDS-tiled kernel only)
    int ones_n;                                   // B(:, N-1) == 1 (appends the bias column to a weight-gradient contraction)
    int epi; float alpha;
    int dbg;                                      // DRIL_GEMM_DBG bits (diagnostic, results wrong): 1 no global operand loads after the first chunk, 2 no MFMA, 4 no epilogue, 8 no staging stores
    int allow_split;                              // large contractions may run on the bf16 matrix cores with fp32-equivalent 3-piece operand splitting (generic on-policy path; SAC keeps the f32 MFMA)
};
enum { EPI_NONE = 0, EPI_RELU = 1, EPI_TANH = 2, EPI_MASK_RELU = 3, EPI_MASK_TANH = 4,
       // round 3: the other activations whose derivative is a function of the OUTPUT (the reverse pass keeps activations, not pre-activations): NNlib sigmoid,
       // elu (alpha = 1), leakyrelu (a = 0.01), softplus — generic PPO path only (the reference takes any activation, layer_constructors.jl:8,56)
       EPI_SIGMOID = 5, EPI_ELU = 6, EPI_LEAKY = 7, EPI_SOFTPLUS = 8, EPI_MASK_SIGMOID = 9, EPI_MASK_ELU = 10, EPI_MASK_LEAKY = 11, EPI_MASK_SOFTPLUS = 12,
       // gelu (NNlib: the tanh form) and swish: the derivative is a function of the PRE-activation, which the forward of an update keeps beside the activation (GemmArgs.zout); their mask epilogues read it as `aux`
       EPI_GELU = 13, EPI_SWISH = 14, EPI_MASK_GELU = 15, EPI_MASK_SWISH = 16 };
__host__ __device__ inline bool epi_reads_aux(int epi) { return epi == EPI_MASK_RELU || epi == EPI_MASK_TANH || (epi >= EPI_MASK_SIGMOID && epi <= EPI_MASK_SOFTPLUS) || epi == EPI_MASK_GELU || epi == EPI_MASK_SWISH; }
inline bool activation_needs_preactivation(int act) { return act == 6 || act == 7; }
// activation codes of dril_config.activation -> the forward epilogue and the mask (act'(y)) epilogue
inline int epi_of_activation(int act) { return act == 1 ? EPI_RELU : act == 2 ? EPI_SIGMOID : act == 3 ? EPI_ELU : act == 4 ? EPI_LEAKY : act == 5 ? EPI_SOFTPLUS : act == 6 ? EPI_GELU : act == 7 ? EPI_SWISH : EPI_TANH; }
inline int mask_epi_of_activation(int act) { return act == 1 ? EPI_MASK_RELU : act == 2 ? EPI_MASK_SIGMOID : act == 3 ? EPI_MASK_ELU : act == 4 ? EPI_MASK_LEAKY : act == 5 ? EPI_MASK_SOFTPLUS : act == 6 ? EPI_MASK_GELU : act == 7 ? EPI_MASK_SWISH : EPI_MASK_TANH; }

GemmArgs gemm_args();

// The kernels launch_gemm picks between, in ONE table: X(id, name, grid shape, kernel).  launch_gemm switches on gemm_select() and launches the kernel of the
// selected row, gemm_target_name() prints the name of the same row (tests/gemm_check.hip --plan, tests/test_gemm_plan.py), so neither can drift from the other.
// Grid shapes (dril_gemm.hip gemm_grid): TILE one workgroup per 32 x 32 tile (its 8 waves split K), ROW8 one per 32 x 256 block (a tile per wave),
// SPLIT2 one per 64 x 256 block (two m-tiles per wave); LDS = TILE with the 66 KB dynamic LDS block.
// lds_<A><B>: access pattern of the staged operand, 0 k-contiguous float4, 1 row-contiguous float4 (GemmArgs.ldsA / ldsB: one kernel, four bodies).
// big / split <am|ak>_<bk|bn>: A m- or k-contiguous, B k- or n-contiguous; split = the bf16 three-piece operand split, mb = m-tiles per wave.
#define DRIL_GEMM_TARGETS(X) \
    X(GEMM_DIRECT_SPLITK, "direct_splitk", GEMM_GRID_TILE, (sac_gemm_kernel<true>)) \
    X(GEMM_DIRECT_TILES, "direct_tiles", GEMM_GRID_ROW8, (sac_gemm_kernel<false>)) \
    X(GEMM_LDS_00, "lds_00", GEMM_GRID_LDS, (sac_gemm_lds_kernel)) \
    X(GEMM_LDS_01, "lds_01", GEMM_GRID_LDS, (sac_gemm_lds_kernel)) \
    X(GEMM_LDS_10, "lds_10", GEMM_GRID_LDS, (sac_gemm_lds_kernel)) \
    X(GEMM_LDS_11, "lds_11", GEMM_GRID_LDS, (sac_gemm_lds_kernel)) \
    X(GEMM_BIG_AM_BK, "big_am_bk", GEMM_GRID_ROW8, (sac_gemm_big_kernel<false, false>)) \
    X(GEMM_BIG_AK_BK, "big_ak_bk", GEMM_GRID_ROW8, (sac_gemm_big_kernel<true, false>)) \
    X(GEMM_BIG_AM_BN, "big_am_bn", GEMM_GRID_ROW8, (sac_gemm_big_kernel<false, true>)) \
    X(GEMM_BIG_AK_BN, "big_ak_bn", GEMM_GRID_ROW8, (sac_gemm_big_kernel<true, true>)) \
    X(GEMM_SPLIT_AM_BK_MB1, "split_am_bk_mb1", GEMM_GRID_ROW8, (sac_gemm_split_kernel<false, false, 1, 1>)) \
    X(GEMM_SPLIT_AK_BK_MB1, "split_ak_bk_mb1", GEMM_GRID_ROW8, (sac_gemm_split_kernel<true, false, 1, 1>)) \
    X(GEMM_SPLIT_AM_BN_MB1, "split_am_bn_mb1", GEMM_GRID_ROW8, (sac_gemm_split_kernel<false, true, 1, 1>)) \
    X(GEMM_SPLIT_AK_BN_MB1, "split_ak_bn_mb1", GEMM_GRID_ROW8, (sac_gemm_split_kernel<true, true, 1, 1>)) \
    X(GEMM_SPLIT_AM_BK_MB2, "split_am_bk_mb2", GEMM_GRID_SPLIT2, (sac_gemm_split_kernel<false, false, 2, 1>)) \
    X(GEMM_SPLIT_AK_BK_MB2, "split_ak_bk_mb2", GEMM_GRID_SPLIT2, (sac_gemm_split_kernel<true, false, 2, 1>)) \
    X(GEMM_SPLIT_AM_BN_MB2, "split_am_bn_mb2", GEMM_GRID_SPLIT2, (sac_gemm_split_kernel<false, true, 2, 1>)) \
    X(GEMM_SPLIT_AK_BN_MB2, "split_ak_bn_mb2", GEMM_GRID_SPLIT2, (sac_gemm_split_kernel<true, true, 2, 1>))
enum GemmTarget {
#define DRIL_GEMM_TARGET_ID(id, name, grid, kernel) id,
    DRIL_GEMM_TARGETS(DRIL_GEMM_TARGET_ID)
#undef DRIL_GEMM_TARGET_ID
    GEMM_TARGET_COUNT
};
enum GemmGrid { GEMM_GRID_TILE, GEMM_GRID_LDS, GEMM_GRID_ROW8, GEMM_GRID_SPLIT2 };
// fills the derived fields (vecA / vecB / vecBn, use_lds, ldsA / ldsB, dbg) from shape, strides and pointer alignment; false: an empty contraction
bool gemm_prepare(GemmArgs& g);
// the split-K body a PREPARED contraction runs on: GEMM_LDS_<ldsA><ldsB> with use_lds, else GEMM_DIRECT_SPLITK.  launch_gemm below its tile-count threshold,
// and launch_gemm_pair / launch_gemm_multi for each of their contractions on its own (gemm_body_any)
inline GemmTarget gemm_splitk_body(const GemmArgs& g) { return g.use_lds ? (GemmTarget)(GEMM_LDS_00 + 2 * g.ldsA + g.ldsB) : GEMM_DIRECT_SPLITK; }
// the kernel launch_gemm runs for a PREPARED contraction of Z batches (a host function of the arguments alone: no device call)
GemmTarget gemm_select(const GemmArgs& g, int Z);
const char* gemm_target_name(GemmTarget t);
// one contraction, Z batches (blockIdx.z); picks the split-K / tile-parallel / LDS-tiled shape from the tile count
hipError_t launch_gemm(GemmArgs g, int Z, hipStream_t s);
// two independent contractions in one launch (a layer's [dW | db] and its dz): blockIdx.z < Za runs `a`
hipError_t launch_gemm_pair(GemmArgs a, int Za, GemmArgs b, int Zb, hipStream_t s);
// up to four independent contractions in one launch (the split-K shape, like the pair): contraction i runs Zs[i] batches
hipError_t launch_gemm_multi(const GemmArgs* gs, const int* Zs, int n, hipStream_t s);

}  // namespace dril
