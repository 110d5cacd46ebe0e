// lr_device.hpp -- device-side parameter blocks and launch plumbing shared by the kernel files.
#pragma once
#include <hip/hip_runtime.h>

#include "lr_arith.hpp"
#include "lr_float128.hpp"

namespace lr {

// per-modulus constants, one entry per limb of a context (device array)
struct LimbParams {
    u64 q;
    u64 qinv;        // q^-1 mod 2^64              (mredParams)
    u64 bred_hi;     // floor(2^128/q) >> 64       (bredParams[0])
    u64 bred_lo;     //                            (bredParams[1])
    u64 n_inv_mont;  // Go's nttNInv (Montgomery form of N^-1)
    u64 n_inv;       // N^-1 mod q, plain
    u64 n_inv_shoup; // floor(n_inv * 2^64 / q)
    // quotient estimate for values < 2^64 when q >= 2^57 (lr_ntt.hip, est_quotient): with
    // qh = (q >> 32) + 1, red_m = min(floor(2^(32+red_g) / qh), 2^32-1), red_g = bitlen(qh) - 1
    u32 red_m;
    u32 red_g;
};

constexpr int kMaxLimbs = 64;

// What a launcher decides from its arguments before it touches the device.  A family's rule is written once, as the launch_verdict next to
// its launch struct; the launcher and its stand-in under tests/cpp both ask it, so the host sanitizer builds check the product's rule.
enum LaunchVerdict { kLaunchGo = 0, kLaunchEmpty, kLaunchRefuse };     // empty: nothing to do, hipSuccess; refuse: hipErrorInvalidValue
inline LaunchVerdict launch_verdict(bool empty, bool bad) { return empty ? kLaunchEmpty : bad ? kLaunchRefuse : kLaunchGo; }
inline hipError_t verdict_error(LaunchVerdict v) { return v == kLaunchRefuse ? hipErrorInvalidValue : hipSuccess; }

// The library's configuration, one copy per handle, fixed when the handle is created: the internal image of the public lr_options
// (include/lattigo_ring.h; from_public / to_public in lr_abi_core.cpp).  A deployment configures through lr_options and the *_create_ex
// entry points; the LR_* environment variables named below are a TEST-ONLY override of the same fields, read in exactly one place
// (apply_env) at handle creation -- a caller's environment cannot change the code path of a live handle in the middle of a run.
struct Options {
    bool no_asm = false;           // LR_NO_ASM: C++ NTT kernels only
    bool no_fp = false;            // LR_NO_FP: integer bodies for every modulus
    bool no_epilogue = false;      // LR_NO_EPILOGUE: separate subtract-multiply instead of the forward kernels' epilogue
    bool no_int_epilogue = false;  // LR_NO_INT_EPILOGUE: the epilogue on the FP64 bodies only (limbs of 2^46 and more keep the separate pass)
    bool rescale_unfused = false;  // LR_RESCALE_UNFUSED: the rounding rescale with explicit shifted copies
    bool no_staging = false;       // LR_NO_STAGING: N = 2^16 key switch with in-place forward transforms
    bool ext_narrow = false;       // LR_EXT_NARROW: per-term basis extension instead of the 128-bit column sums
    bool asm14_1024 = false;       // LR_ASM_14_1024: the 1024-thread plan at N = 2^14
    bool timeline = false;         // LR_NTT_TIMELINE: plain 2^15 launches (forward / inverse, integer variant 1 and dual variant 3) run the stamped diagnostics builds
    bool keymac_narrow = false;    // LR_KEYMAC_NARROW: one Montgomery product per term in the key inner product instead of the 128-bit sums
    bool no_invfuse = false;       // LR_NO_INVFUSE: N = 2^16 inverse transforms as lazy sub-blocks + the separate last-stage pass (ntt_top_kernel) instead of the pair-flag kernels
    bool no_wide14_small = false;  // LR_ASM_14_NO_WIDE_SMALL: the 512-thread plan at N = 2^14 for small launches too
    bool no_invtop = false;        // LR_NO_INVTOP: the inverse transforms in front of a top-stage extension finish with their own last-stage pass
    bool no_ext_chunks = false;    // LR_NO_EXT_CHUNKS: a basis extension of a small batch as one launch over all target columns instead of column ranges on grid z
    bool no_pair = false;          // LR_NO_PAIR: ModDown's two components of a single ciphertext as two launches instead of one with distance strides
    bool rescale_unpaired = false; // LR_RESCALE_UNPAIRED: lr_ckks_rescale divides the two components one after the other at every batch size
    int split15 = -1;              // LR_NTT_SPLIT15: N = 2^15 transforms as two 2^14 sub-blocks: 0 never, 1 always, unset = launches of at most kSplit15Below workgroups
    bool no_fork = false;          // LR_NO_FORK: the key switch's independent launches in order on one stream at every batch size
    bool no_ext_group = false;     // LR_NO_EXT_GROUP: one extension launch per key-switch digit instead of one grouped launch
    bool no_exttop = false;        // LR_NO_EXTTOP: N = 2^16 key switch with staged extensions and fused-top transforms instead of the top stage inside the extension
    int persist = -1;              // LR_NTT_PERSIST: polys per workgroup of the persistent forward 2^15 kernels (0 = one-poly workgroups, -1 = default)
    int stagger = -1;              // LR_NTT_STAGGER: start-up stagger of the assembly NTT kernels in kilo-clocks per step (0 = off)
    int ntt_mode = -1;             // LR_NTT_MODE
    int asm_variant = -1;          // LR_ASM_VARIANT
    bool ext_ieee_div = false;     // LR_EXT_IEEE_DIV: IEEE division in the extension's float correction (the reference-shaped kernel)
    bool no_grid_padding = false;  // LR_NTT_NO_GRID_PADDING: assembly launches with the limb count on grid x unpadded
    bool bfv_no_ext_epilogue = false;  // LR_BFV_NO_EXT_EPILOGUE
    bool bfv_no_gather = false;    // LR_BFV_NO_GATHER
    // launch-shape thresholds (measured defaults: DESIGN.md decision table)
    int split15_max_workgroups = 128;   // LR_NTT_SPLIT15_BELOW: N = 2^15 launches of at most this many workgroups run as 2^14 sub-blocks
    int wide14_max_items = 256;         // N = 2^14 launches of at most this many transforms use the 1024-thread kernels
    int pair_max_workgroups = 256;      // two components of one ciphertext / the Q and P parts of one inner product as one launch up to here
    int fork_below_workgroups = 256;    // LR_FORK_BELOW: a lone plan forks a launch below this many workgroups
    long long bfv_gather_below = 1536;  // LR_BFV_GATHER_BELOW
    bool bfv_encoder_unfused = false;   // LR_BFV_ENCODER_UNFUSED: the encoder's composed route where the fused kernels would run
    bool ckks_encoder_tiled = false;    // LR_CKKS_ENCODER_TILED: the CKKS encoder's tiled route where the fused kernels would run
    void apply_env();              // the test-only override: the ONE place that reads LR_* variables
    static Options from_env() {    // defaults + the override: what the plain *_create entry points use
        Options o;
        o.apply_env();
        return o;
    }
};
// small per-limb host values travelling in the kernel-argument segment (no host->device copy)
struct LimbScalars { u64 v[kMaxLimbs]; };

// a twiddle factor in the kernels' internal form: x = psi power (plain domain), y = floor(x*2^64/q)
typedef ulonglong2 Twiddle;

constexpr u64 kFpLimit = 1ull << 46;
// per-limb constants of the FP64 butterflies (moduli below 2^46); q = 0.0: the limb stays on the integer body
struct FpLimb {
    double q, q_inv;            // q and RN(1/q)
    double n_inv, n_inv_q;      // N^-1 mod q and RN(n_inv / q): the scaling of the inverse transform
};

// constant of the forward kernels' epilogue, 16 bytes per limb: (c, RN(c / q)) as doubles for a limb the FP64 body takes, the Shoup pair
// (c, floor(c 2^64 / q)) as two u64 in the same bytes for a limb on an integer body (make_epi_limb, lr_abi_ring.cpp)
struct EpiLimb { double c, c_over_q; };

// Addressing of one NTT launch.  Work item (b, i): batch element b, i-th limb of the launch.
struct NttLaunch {
    const u64 *in;
    u64 *out;
    long long in_poly_stride;   // u64 elements between consecutive batch polys
    long long out_poly_stride;
    int in_limb0, in_limb_step;   // input row  = in_limb0  + i * in_limb_step
    int out_limb0, out_limb_step; // output row = out_limb0 + i * out_limb_step
    int mod0, mod_step;           // modulus    = mod0      + i * mod_step
    int n_items;                  // limbs per poly in this launch
    int batch;
    const LimbParams *lp;       // [L]
    const Twiddle *tw;          // [L][N] forward or inverse table
    const Twiddle *tw_fin;      // [L][15][N/16] lane-transposed copy of the last four stages (N >= 2^12), or null
    int sub_log;                // log2(sub-blocks per limb): 0, or 1 when N = 2^16 runs as two 2^15 sub-transforms
    // digit groups (key switching): batch = groups * group polys; the polys of group g skip the items
    // [g*hole, (g+1)*hole): item = i + (i >= g*hole ? hole : 0), i < n_items.  hole = 0: plain launch.
    int hole;
    int group;
    int fuse_top;               // sub_log = 1, forward, out of place: the sub-transforms compute the stage over bit 15 while
                                // loading (each reads both halves of the limb), no separate streaming pass.
                                // Persistent kernels (lr_ntt_fwd15p_*, sub_log = 0): polys per workgroup; grid y (x for the dual
                                // kernels) counts chunks of that many polys inside a group, and `group` is set for plain launches too
    // dual assembly kernels ("m3"): a limb whose fp_lp entry is set runs on the FP64 body, with twiddles (w, RN(w/q)) as
    // doubles in tables laid out exactly like tw / tw_fin, found at tw + fp_tw_delta / tw_fin + fp_fin_delta (bytes)
    long long fp_tw_delta, fp_fin_delta;
    const FpLimb *fp_lp;        // [L], or null for every other kernel
    // epilogue kernels ("m4", forward, FP64 limbs only): out = (x - NTT(in)) * c + plus (mod q), x and plus laid out like the
    // output rows (row = out_limb0 + i * out_limb_step) with their own strides between polys
    const u64 *epi_x;
    long long epi_x_stride;
    const u64 *epi_plus;
    long long epi_plus_stride;
    const EpiLimb *epi_consts;  // [L]: per limb (c, RN(c / q)) as doubles or the Shoup pair of c (EpiLimb), indexed like lp
    // assembly kernels: start-up stagger of the first round of workgroups (gen_ntt.py: stagger), set by the launcher
    int stagger_gx;             // the grid's x extent (linear workgroup id = x + stagger_gx * y)
    int stagger_unit;           // kilo-clocks per step of the 16-step start offset; 0 = all workgroups start at once
};
static_assert(sizeof(NttLaunch) == 176, "NttLaunch layout is shared with asmgen/gen_ntt.py (fields are read at fixed offsets)");

// ---- coefficient-wise launches (lr_ewise.hip) ----
struct EwiseLaunch {
    const u64 *a;
    const u64 *b;
    u64 *out;
    long long a_stride, b_stride, out_stride;  // u64 elements between batch polys (0 = broadcast)
    int n;                                      // ring degree
    const LimbParams *lp;
    int has_scalars;
    LimbScalars scalars;                        // per limb, pre-processed per op on the host
};

// out = MRed(a + (q - b), consts[limb])
struct SubMulLaunch {
    const u64 *a;
    const u64 *b;
    u64 *out;
    long long a_stride, b_stride, out_stride;
    long long b_row_stride;  // n, or 0 when every limb subtracts the same row (the last limb, ring_scaling.go:41)
    int n;
    const LimbParams *lp;
    const u64 *consts;  // device [limbs], Montgomery form
    int reduce_b;       // 1: b is first reduced with BRedAdd (coefficient-domain rescale, ring_scaling.go:50,146)
    LimbScalars addend; // b + addend[limb] before the reduction (pHalfNegQi); zeros when unused
    const u64 *plus;    // optional: out = CRed(plus + result) (the Context.Add that follows a ModDown in ckks MulRelin)
    long long plus_stride;
    int has_post;       // 1: out = CRed(result + post[limb]) (the AddScalarBigint that follows ModDownSplitedQP in bfv Mul)
    LimbScalars post;
};

// out = MRed(CRed(x + (q - sub[limb])), mul[limb]): SubScalarBigint then MulScalar (bfv/evaluator.go:459,462) in one pass
struct ScalarPairLaunch {
    const u64 *in;
    u64 *out;
    long long in_stride, out_stride;
    int n;
    const LimbParams *lp;
    LimbScalars sub, mul;
};
hipError_t launch_scalar_pair(const ScalarPairLaunch &L, int limbs, int batch, hipStream_t stream);

// degree-2 tensor product of two degree-1 ciphertexts (ckks/evaluator.go:1080-1095) in one pass
struct TensorLaunch {
    const u64 *a0, *a1, *b0, *b1;
    long long a0_stride, a1_stride, b0_stride, b1_stride;
    u64 *c0, *c1, *c2;        // may alias the inputs (every thread reads its four operands before it writes)
    long long c_stride;       // of c0
    int n;
    const LimbParams *lp;
    long long c1_stride, c2_stride;
    const u64 *const *table = nullptr;   // batcher form: the operands of batch poly b are table[4b .. 4b+3] (a0, a1, b0, b1), a*/b* and their strides unused
};
hipError_t launch_tensor(const TensorLaunch &L, int limbs, int batch, hipStream_t stream);

// the tensor of bfv tensorAndRescale for operands that are not both of degree 1 (bfv/evaluator.go:371-415) in one pass: c[i+j] accumulates
// MRed(MForm(a_i), b_j) with CRed (MulCoeffsMontgomeryAndAdd), or, squaring (a == b, degree 2 only), c[i+j] = 2 MRed(MForm(a_i), a_j) for
// i < j and c[2i] += MRed(MForm(a_i), a_i).  Every accumulator is canonical, so the order of the terms does not change a bit.
constexpr int kTensorMaxDegree = 5;     // d0 + d1 <= 5: bfv.NewEvaluator's pools hold 6 polys (bfv/evaluator.go:74-82)
struct TensorDegLaunch {
    const u64 *a[kTensorMaxDegree + 1];   // a[0..d0]
    const u64 *b[kTensorMaxDegree + 1];   // b[0..d1] (unread when squaring)
    u64 *c[kTensorMaxDegree + 1];         // c[0..d0+d1]; may alias an operand (every thread reads its operands before it writes)
    long long stride;                     // between batch polys, operands and products alike
    int n;
    const LimbParams *lp;
};
// d0, d1 >= 0, 1 <= d0 + d1 <= 5, (d0, d1) != (1, 1) (that is launch_tensor); square only with d0 == d1 == 2; else hipErrorInvalidValue
hipError_t launch_tensor_deg(const TensorDegLaunch &L, int d0, int d1, bool square, int limbs, int batch, hipStream_t stream);
inline LaunchVerdict launch_verdict(const TensorDegLaunch &, int d0, int d1, bool square, int limbs, int batch) {      // (refusals first: a bad degree is an error at any size)
    const bool bad = d0 < 0 || d1 < 0 || d0 + d1 < 1 || d0 + d1 > kTensorMaxDegree || (d0 == 1 && d1 == 1) || (square && !(d0 == 2 && d1 == 2));
    return bad ? kLaunchRefuse : (limbs <= 0 || batch <= 0) ? kLaunchEmpty : kLaunchGo;
}

// decryptor.Decrypt (ckks/decryptor.go:53-78) in one pass: Horner evaluation of ct[0..degree] at the secret key with the reference's
// element operations and reduction cadence -- acc = ct[degree]; for i = degree..1: acc = CRed(MRed(acc, sk) + ct[i-1]), BRedAdd when
// i & 7 == 7; a final BRedAdd unless degree & 7 == 7 -- every operand read once, the result written once
constexpr int kHornerMaxDegree = 8;
struct HornerLaunch {
    const u64 *ct[kHornerMaxDegree + 1];
    long long ct_stride[kHornerMaxDegree + 1];
    const u64 *sk;
    long long sk_stride;            // 0: one key for the whole batch
    u64 *out;
    long long out_stride;
    int degree, n;
    const LimbParams *lp;
};
hipError_t launch_horner(const HornerLaunch &L, int limbs, int batch, hipStream_t stream);

// out0 = MRed(a, b0), out1 = MRed(a, b1): the two products of pkEncryptor.encrypt with the public key (ckks/encryptor.go:209-211) reading u once
struct Mul2Launch {
    const u64 *a, *b0, *b1;
    u64 *out0, *out1;
    long long a_stride, b0_stride, b1_stride, out0_stride, out1_stride;     // between batch polys (0 = broadcast)
    int n;
    const LimbParams *lp;
};
hipError_t launch_mul2(const Mul2Launch &L, int limbs, int batch, hipStream_t stream);

// batcher form of a result copy: dst[b] = table[b * per_poly + k] for the per_poly staged polys src[k] (rows [limbs][n], batch stride `stride`)
struct ScatterLaunch {
    const u64 *src[4];          // per_poly <= 4 of them are used
    long long stride;
    u64 *const *table;
    int per_poly, n;
};
hipError_t launch_scatter(const ScatterLaunch &L, int limbs, int batch, hipStream_t stream);
// the other way round (the BFV batcher's operands): dst[k] + b * stride <- table[b * per_poly + k], k < per_poly <= 4
struct GatherLaunch {
    u64 *dst[4];
    long long stride;
    const u64 *const *table;
    int per_poly, n;
};
hipError_t launch_gather(const GatherLaunch &L, int limbs, int batch, hipStream_t stream);

// up to eight polys with unrelated addresses copied to / from the slots of one contiguous buffer (BFV Mul at a small batch: the four
// operand polys become one batch of 4 B, the three results leave one batch of 3 B; other degrees gather up to 7 operand polys and
// scatter up to 6 results: bfv_tensor_and_rescale, lr_abi_bfv.cpp): poly k = z / batch, batch element z % batch; slots from `count` on are not read
constexpr int kMultiCopyMax = 8;
struct MultiCopyLaunch {
    const u64 *src[kMultiCopyMax];
    long long src_stride[kMultiCopyMax];
    u64 *dst[kMultiCopyMax];
    long long dst_stride[kMultiCopyMax];
    int count, batch, n;
};
hipError_t launch_multicopy(const MultiCopyLaunch &L, int limbs, hipStream_t stream);

// out_row[r] = in + adds[r] (optionally CRed)
struct RowAddLaunch {
    const u64 *in;   // one row per batch poly
    u64 *out;
    long long in_stride, out_stride;
    int n;
    u64 q;           // 0: no reduction
    LimbScalars adds; // per output row
};

// half-vector scalar operations (the constant-by-ciphertext methods of ckks.Evaluator, ckks/evaluator.go:373-830): coefficients
// j < n/2 of limb i take the scalar lo[i], the others hi[i] (in the NTT domain the two halves are the slots' real and
// imaginary... conjugate positions: x^(n/2) acts as +i on one half and -i on the other)
struct HalfScalarLaunch {
    const u64 *in;
    u64 *out;
    long long in_stride, out_stride;
    int n;
    int op;                 // 0: out = CRed(in + s)   1: out = MRed(in, s)   2: out = CRed(out + MRed(in, s))
    const LimbParams *lp;
    LimbScalars lo, hi;
};

// res = c0 + sum c_k ct_k (lr_ckks_eval.hip): evaluatePolyFromPowerBasis' chain AddConst, MultByConstAndAdd ... (ckks/
// polynomial_evaluation.go:142-159) on both components of a degree-1 ciphertext in one pass.  Per limb, coefficient j and component u:
//   acc = accumulate ? out_u : 0;  component 0 with has_add: acc = CRed(acc + (j < n/2 ? add_lo : add_hi))
//   for k < count: bit k of pre_mask: acc = MRed(acc, pre_k);  acc = CRed(acc + MRed(x_k,u, j < n/2 ? lo_k : hi_k))
// -- HalfScalarLaunch's op 0, then per term op 1 and op 2, with the accumulator in registers.  The constants travel in the kernel
// arguments (no table on the device, no copy, nothing to synchronise; a captured launch carries them): per limb of the launch
// lincomb_limb_words words in `k` -- add_lo, add_hi when has_add, then (pre, lo, hi) per term -- so a launch covers
// lincomb_limbs_per_launch limbs from limb0 on and a workgroup reads its own limb's words at wave-uniform addresses.
constexpr int kLinCombTerms = 16;        // terms whose addresses travel in one launch
constexpr int kLinCombWords = 384;       // words of constants in one launch: eight limbs of sixteen terms
struct LinCombTermRef {
    const u64 *c[2];
    long long stride[2];                 // between batch polys
};
struct LinCombLaunch {
    LinCombTermRef term[kLinCombTerms];
    u64 *out[2];
    long long out_stride[2];
    int n, count, limb0, accumulate, has_add;
    unsigned pre_mask;
    const LimbParams *lp;
    u64 k[kLinCombWords];
};
static_assert(sizeof(LinCombLaunch) <= 4096, "LinCombLaunch travels by value in the kernel arguments");
LR_HD int lincomb_limb_words(int count, int has_add) { return 3 * count + (has_add ? 2 : 0); }
inline int lincomb_limbs_per_launch(int count, int has_add) {
    const int w = lincomb_limb_words(count, has_add);
    return w == 0 || kLinCombWords / w > kMaxLimbs ? kMaxLimbs : kLinCombWords / w;
}
hipError_t launch_ckks_lincomb(const LinCombLaunch &L, int limbs, int batch, hipStream_t stream);
// (component on grid z next to the batch member: 2 * batch <= 65535)
inline LaunchVerdict launch_verdict(const LinCombLaunch &L, int limbs, int batch) {
    return launch_verdict(limbs <= 0 || batch <= 0, L.n < 4 || L.count < 0 || L.count > kLinCombTerms || L.limb0 < 0 || L.limb0 + limbs > kMaxLimbs ||
                                                        limbs > lincomb_limbs_per_launch(L.count, L.has_add) || batch > 32767);
}

// out = a (+|-) b over CKKS ciphertexts of any degree (lr_ckks_eval.hip): the element loops of evaluator.Add / AddNoMod / Sub / SubNoMod
// through evaluateInPlace (ckks/evaluator.go:227-342) with Sub's NegLvl tail (:186-192, :203-209), in one pass.  Per limb, coefficient j
// and component u <= max(deg_a, deg_b), with s(j) = j < n/2 ? lo : hi:
//   x = a_u (u <= deg_a), y = b_u (u <= deg_b; deg_b = -1: no b);  double_a: x = CRed(x + x);  mult_a: x = MRed(x, ma(j));
//   mult_b: y = MRed(y, mb(j));  both: r = op(x, y);  only x: r = x;  only y: r = y, or q - y for the two subtractions;
//   component 0 with has_add: r = CRed(r + add(j))
// The constants travel in the kernel arguments, kCombineLimbWords per limb (ma_lo, ma_hi, mb_lo, mb_hi, add_lo, add_hi; zero where the
// flag is off): kMaxLimbs limbs fill LinCombLaunch's budget of kLinCombWords exactly, so every level is one launch.
constexpr int kCombineLimbWords = 6;
constexpr int kCombineComps = 3;         // components of a ciphertext of degree 2
static_assert(kCombineLimbWords * kMaxLimbs <= kLinCombWords, "every limb's words in one launch");
struct CombineLaunch {
    const u64 *a[kCombineComps], *b[kCombineComps];
    u64 *out[kCombineComps];
    long long a_stride[kCombineComps], b_stride[kCombineComps], out_stride[kCombineComps];     // between batch polys; 0: one poly read by every member
    int n, op;                           // op: LR_ADD, LR_ADD_NOMOD, LR_SUB, LR_SUB_NOMOD
    int deg_a, deg_b;                    // deg_a in 0..2, deg_b in -1..2
    int double_a, mult_a, mult_b, has_add;
    const LimbParams *lp;
    u64 k[kCombineLimbWords * kMaxLimbs];
};
static_assert(sizeof(CombineLaunch) <= 4096, "CombineLaunch travels by value in the kernel arguments");
LR_HD int combine_comps(int deg_a, int deg_b) { return (deg_a > deg_b ? deg_a : deg_b) + 1; }
hipError_t launch_ckks_combine(const CombineLaunch &L, int limbs, int batch, hipStream_t stream);
// (component on grid z next to the batch member: comps * batch <= 65535, which batch <= 32767 ensures up to degree 1)
inline LaunchVerdict launch_verdict(const CombineLaunch &L, int limbs, int batch) {
    return launch_verdict(limbs <= 0 || batch <= 0, L.n < 4 || L.op < 0 || L.op > 3 || L.deg_a < 0 || L.deg_a >= kCombineComps || L.deg_b < -1 ||
                                                        L.deg_b >= kCombineComps || limbs > kMaxLimbs || batch > 32767 ||
                                                        (long long)combine_comps(L.deg_a, L.deg_b) * batch > 65535);
}

// key-switch inner product over all digits (lr_ewise.hip)
struct KeyMacLaunch {
    const u64 *c2;                 // [beta][batch][limbs][N], NTT domain
    long long c2_digit_stride;     // u64 elements between digits
    long long c2_poly_stride;      // between batch polys
    const u64 *key;                // SwitchingKey image [2*beta][key limbs][N] (NTT + Montgomery form)
    long long key_poly_stride;     // between key polys
    int key_limb0;                 // first key limb of this segment (0 for Q, |Q| for P)
    u64 *out0, *out1;
    long long out_stride;          // of out0
    int n, beta;
    const LimbParams *lp;
    // limbs [i*alpha, (i+1)*alpha) of digit i are the NTT-domain input itself (ckks/evaluator.go:1579-1584):
    // read from `own` (poly stride own_stride) instead of a copy inside c2; alpha = 0 disables
    const u64 *own;
    long long own_stride;
    int alpha;
    long long out1_stride;         // of out1 (the two outputs of lr_ckks_switch_keys may have different allocations)
    int tile8;                     // set by the launcher: grid x = poly * 8 + (chunk mod 8) (one XCD per key tile)
    int wide;                      // 1: exact 128-bit sums + one Montgomery reduction per output (needs beta * max q < 2^64, q < 2^61)
    // hoisted rotations (ckks/evaluator.go:1346-1347): the digits are read THROUGH ring.PermuteNTT's index for the Galois element perm_gen
    // (reduced modulo 2N; 0 = as they are) instead of from permuted copies; needs own == nullptr (the digits carry their own limbs)
    unsigned perm_gen;
    int logn;
};
hipError_t launch_keymac(const KeyMacLaunch &L, int limbs, int batch, hipStream_t stream);
// the Q part and the P part of one inner product as ONE launch (grid y = limbs_a + limbs_b; both wide, same beta): two launches of a
// small batch run one after the other although they share nothing; hipErrorNotSupported: launch them separately
struct KeyMacPair {
    KeyMacLaunch a, b;
    int split;                     // grid y < split: a with limb y; otherwise b with limb y - split
};
hipError_t launch_keymac_pair(const KeyMacLaunch &A, int limbs_a, const KeyMacLaunch &B, int limbs_b, int batch, hipStream_t stream);

// Poly.MarshalBinary payload (ring/ring_object.go:146-156,197-207): big-endian words <-> device rows
hipError_t launch_bswap(const u64 *in, u64 *out, size_t words, hipStream_t stream);

// ring/ring_galois.go
struct GaloisLaunch {
    const u64 *in;
    u64 *out;
    long long in_stride, out_stride;
    int n, logn;
    int ntt_domain;    // 1: PermuteNTT gather, 0: Context.Permute scatter with sign
    u64 gen;           // reduced modulo 2N
    const LimbParams *lp;
    const u64 *const *in_table = nullptr;   // batcher form: batch poly b is read from in_table[b] (in / in_stride unused)
};
hipError_t launch_permute(const GaloisLaunch &L, int limbs, int batch, hipStream_t stream);
// the degrees whose coefficient-domain rows one workgroup holds in LDS (permute_coeff_lds_kernel, bfv_chain_step_kernel): 128 KiB of the
// CU's 160 at N = 2^14; below 2^11 a row is too short to pay for a workgroup of its own
inline bool lds_row_degree(int logn) { return logn >= 11 && logn <= 14; }
// g^-1 modulo 2N for an odd g (Newton's iteration doubles the correct low bits): output j of Context.Permute is input (j * g^-1 mod 2N) mod N
inline u32 galois_inverse(u64 gen, int n) {
    const u32 mask2 = 2u * (u32)n - 1u, g = (u32)gen & mask2;
    u32 inv = g;
    for (int it = 0; it < 5; ++it) inv *= 2u - g * inv;
    return inv & mask2;
}

// One step of a BFV rotation chain after its key switch (lr_bfv_rotate_chain, lr_bfv_inner_sum; bfv/evaluator.go:711-733 followed by
// InnerSum's Add :703 / :707, or nothing for rotateColumnsPow2 :657): see bfv_chain_step_kernel.  Coefficient domain, all of Q.
struct BfvChainStepLaunch {
    const u64 *a0, *a1;      // the chain's state before the step
    long long a0_stride, a1_stride;
    const u64 *p0, *p1;      // switchKeys(Permute(a1, g)): the key switch's two results
    long long p_stride;
    u64 *out0, *out1;        // the state after the step; out_k may be p_k or a_k (the pass is row-local), never the other component's operand
    long long out0_stride, out1_stride;
    u64 *cx_next;            // Permute(out1, g'), the next step's key-switch input; nullptr: the last step
    long long cx_stride;
    int n, logn;
    u32 ginv, ginv_next;     // g^-1, g'^-1 modulo 2N (galois_inverse)
    int accumulate;          // 1: InnerSum (the state is added to the rotation), 0: rotateColumnsPow2 (replaced by it)
    const LimbParams *lp;
};
inline LaunchVerdict launch_verdict(const BfvChainStepLaunch &L, int limbs, int batch) {
    return launch_verdict(limbs <= 0 || batch <= 0, !lds_row_degree(L.logn) || (1 << L.logn) != L.n || limbs > kMaxLimbs || batch > 65535 || !(L.ginv & 1u) ||
                                                        (L.cx_next && !(L.ginv_next & 1u)) || L.out0 == L.out1);
}
hipError_t launch_bfv_chain_step(const BfvChainStepLaunch &L, int limbs, int batch, hipStream_t stream);

// The additions of bfv.evaluator.Relinearize after a pass of key switches (lr_bfv_relinearize_deg; bfv/evaluator.go:494-495 once per degree
// of the pass): out[k] = CRed(... CRed(CRed(base[k] + p[k][0]) + p[k][1]) ... + p[k][terms - 1]) for both components k in one launch, see
// bfv_relin_fold_kernel.  Term t of batch member b is the row block p[k] + t * group_stride + b * p_stride: the pass's accumulator, whose
// groups lie group_stride words apart, the highest degree first.  Coefficient domain, all of Q.
constexpr int kBfvRelinFoldTerms = 4;       // degree 5: the key switches of ct[5] .. ct[2]
struct BfvRelinFoldLaunch {
    const u64 *base[2];      // the running pair: ct[0] / ct[1] for the first pass, the outputs afterwards
    long long base_stride[2];
    const u64 *p[2];         // the key switches' results of the pass
    long long p_stride, group_stride;
    int terms;               // 1 .. kBfvRelinFoldTerms
    u64 *out[2];             // out[k] may be base[k] (a lane reads everything before it stores), never the other component's operand
    long long out_stride[2];
    int n;
    const LimbParams *lp;
};
inline LaunchVerdict launch_verdict(const BfvRelinFoldLaunch &L, int limbs, int batch) {
    return launch_verdict(limbs <= 0 || batch <= 0, L.n < 2 || limbs > kMaxLimbs || batch > 32767 || L.terms < 1 || L.terms > kBfvRelinFoldTerms ||
                                                        L.out[0] == L.out[1] || L.out[0] == L.base[1] || L.out[1] == L.base[0]);
}
hipError_t launch_bfv_relin_fold(const BfvRelinFoldLaunch &L, int limbs, int batch, hipStream_t stream);

// One step of an accumulating CKKS rotation chain in front of its key switch (lr_ckks_rotate_chain; the two PermuteNTT calls of
// permuteNTT, ckks/evaluator.go:1458-1459, and the first component's half of the Add that follows the rotation in the slot-sum loop):
// see ckks_chain_step_kernel (lr_ckks_eval.hip).  NTT domain, limbs 0 .. level.
struct CkksChainStepLaunch {
    const u64 *a0, *a1;      // the chain's state before the step
    long long a0_stride, a1_stride;
    u64 *plus0;              // CRed(PermuteNTT(a0, g) + a0): the addend of the key switch's first component
    u64 *cx;                 // PermuteNTT(a1, g): the key switch's input
    long long plus_stride, cx_stride;
    int n, logn;
    u32 gen;                 // g, odd, reduced modulo 2N
    const LimbParams *lp;
};
// (a gather: no output is an input; batch and component share grid z)
inline LaunchVerdict launch_verdict(const CkksChainStepLaunch &L, int limbs, int batch) {
    return launch_verdict(limbs <= 0 || batch <= 0, L.logn < 1 || L.logn > 30 || (1 << L.logn) != L.n || limbs > kMaxLimbs || batch > 32767 || !(L.gen & 1u) ||
                                                        L.gen >= 2u * (u32)L.n || L.plus0 == L.cx || L.plus0 == L.a0 || L.plus0 == L.a1 || L.cx == L.a0 ||
                                                        L.cx == L.a1);
}
hipError_t launch_ckks_chain_step(const CkksChainStepLaunch &L, int limbs, int batch, hipStream_t stream);

// The tail of the products of one chunk of a CKKS power basis (lr_ckks_power_basis; the steps after MulRelin and Rescale in
// computePowerBasis / computePowerBasisCheby, ckks/chebyshev_evaluation.go:92-99): see basis_tail_kernel (lr_ckks_eval.hip).  The chunk's
// `products * batch` members lie back to back in the staging pair, first components then second ones; what differs per product travels
// in a device table: one BasisTailProduct each, then `products` rows of `row` multiplier words, then as many rows of addend words.
struct BasisTailProduct {
    u64 *out[2];             // C[n]'s two polys
    long long out_stride;    // between their batch members (one stride for both)
    int tail;                // 0 copy | 1: 2 x - C[1] | 2: 2 x + const
    int mult_side;           // tail 1: 0 none | 1: x is multiplied | 2: C[1] is
};
struct BasisTailLaunch {
    const u64 *stage;                  // [2][members][stage_stride]
    long long stage_stride;
    const u64 *c1[2];                  // C[1], the subtrahend of tail 1
    long long c1_stride[2];
    const BasisTailProduct *products;  // device, [products]
    const u64 *mult, *add;             // device, [products][row] each
    int row, batch, n;
    const LimbParams *lp;
};
// (member and component share grid z; the staging pair is never an output: the host code hands out a pool of its own)
inline LaunchVerdict launch_verdict(const BasisTailLaunch &L, int limbs, int products) {
    return launch_verdict(limbs <= 0 || products <= 0, L.n < 2 || (L.n & 1) || limbs > kMaxLimbs || limbs > L.row || L.batch < 1 ||
                                                           (long long)products * L.batch > 32767 || !L.stage || !L.products || !L.mult || !L.add);
}
hipError_t launch_ckks_basis_tail(const BasisTailLaunch &L, int limbs, int products, hipStream_t stream);
// Context.MultByMonomial (ring/ring.go:663): out = in * X^shift in Z_q[X]/(X^N+1), shift already reduced modulo 2N;
// like the reference, negated coefficients are q - x without reduction (0 becomes q).  Not in place.
hipError_t launch_monomial(const GaloisLaunch &L, int limbs, int batch, hipStream_t stream);

// SimpleScaler.Scale (ring/ring_scaling.go:275-300): one thread per coefficient reconstructs round(t/Q * x) mod t from all
// limbs of the input (integer parts in Z_t, fractional parts in double-double) and writes it to every limb of the output
struct ScaleLaunch {
    const u64 *in;
    u64 *out;
    long long in_stride, out_stride;   // between batch polys, in words
    const u64 *wi;                     // [limbs_in]
    const double *ti;                  // [limbs_in][2] (hi, lo)
    u64 t, add_param, mul_param;
    int pow2, limbs_in, limbs_out, n;
};
hipError_t launch_simple_scale(const ScaleLaunch &L, int batch, hipStream_t stream);

// ---- bfv.Encoder (lr_bfv_encode.hip): EncodeUint / EncodeInt / DecodeUint / DecodeInt of bfv/encoder.go for a batch of plaintexts ----
// a power of psi modulo a plaintext modulus t < 2^31 in 32-bit Shoup form: w plain, ws = floor(w 2^32 / t)
struct Tw32 { u32 w, ws; };
// what both routes share: indexMatrix (bfv/encoder.go:36-58) and the plaintext modulus with floor(2^64 / t) (BRedParams(t)[0])
struct EncoderTables {
    const u32 *index;      // [N]
    u64 t, t_bred_hi;
    int n, logn;
};
// fused routes, one workgroup per plaintext, the transform over Z_t in LDS (N <= 2^15, t < 2^31)
struct EncodeLaunch {
    EncoderTables tab;
    const void *values;    // device [batch][n_values] uint64 or int64
    long long n_values;
    int is_signed;
    const Tw32 *tw_inv;    // [N]: the [t] context's nttPsiInv out of Montgomery form
    Tw32 n_inv;
    u64 *out;              // plaintext polys over Q, coefficient domain
    long long out_stride;
    int limbs;
    const LimbParams *lp;  // of contextQ
    const u64 *delta_mont; // [limbs] MForm(floor(Q / t) mod q_i), bfv/utils.go:9-23
};
hipError_t launch_bfv_encode_fused(const EncodeLaunch &L, int batch, hipStream_t stream);
struct DecodeLaunch {
    EncoderTables tab;
    const u64 *in;         // [batch][N]: SimpleScaler's one-limb output, values below t
    const Tw32 *tw_fwd;    // [N]: nttPsi out of Montgomery form
    void *values;          // device [batch][N] uint64, or int64 centred around 0 (is_signed)
    int is_signed;
};
hipError_t launch_bfv_decode_fused(const DecodeLaunch &L, int batch, hipStream_t stream);
// composed routes (any t the [t] context takes): the steps around lr_intt / lr_ntt of that context on rows of [batch][N] words
// row[indexMatrix[i]] = values[i] mod t (the residue in [0, t) of a negative value), zero from n_values on
hipError_t launch_bfv_slot_scatter(const EncoderTables &tab, const void *values, long long n_values, int is_signed, u64 *row, int batch, hipStream_t stream);
// out[b][i][j] = MRed(row[b][j], delta_mont[i], q_i): encodePlaintext's loop (bfv/encoder.go:127-136)
hipError_t launch_bfv_lift(const u64 *row, int n, u64 *out, long long out_stride, int limbs, const LimbParams *lp, const u64 *delta_mont, int batch, hipStream_t stream);
// values[b][i] = row[b][indexMatrix[i]], minus t above t >> 1 for the signed form (bfv/encoder.go:148-150, 170-178)
hipError_t launch_bfv_slot_gather(const EncoderTables &tab, const u64 *row, void *values, int is_signed, int batch, hipStream_t stream);

// ---- bfv.Encryptor (lr_bfv_encrypt.hip): the samplers' compact decisions expanded on the device, and the sk product ----
// sampleTernary at p = 0.5 (ring/ternarySampler.go:157-177) from its two bit planes: coefficient i takes bit i & 7 of byte i >> 3 of each
// plane, index = (coeff & (sign ^ 1)) | ((sign & coeff) << 1) into matrixTernaryMontgomery[limb] = {0, MForm(1), MForm(q - 1)}
// (ring/ring_context.go:119-122); one pass writes every limb of the launch
struct TernaryLaunch {
    const unsigned char *coeff_bits, *sign_bits;   // device [batch][n / 8]
    u64 *out;
    long long out_stride;
    int n;
    LimbScalars one, minus_one;                    // rows 1 and 2 of the matrix, per limb of the launch
};
hipError_t launch_bfv_ternary(const TernaryLaunch &L, int limbs, int batch, hipStream_t stream);
inline LaunchVerdict launch_verdict(const TernaryLaunch &L, int limbs, int batch) {
    return launch_verdict(limbs <= 0 || batch <= 0, L.n < 8 || limbs > kMaxLimbs);
}
// the Gaussian samplers' (magnitude, sign) bytes: low 7 bits the magnitude c, bit 7 the sign; the residue is the reference's
// (ring/gaussianSampler.go:247,271): sign 1 -> c, sign 0 -> q - c (so (0, sign 0) is q).  add = 1: out = CRed(x + residue) (Context.Add,
// SampleAndAdd), then CRed(. + plus) where a component has a `plus` (the Context.Add of the plaintext that ends encrypt); add = 0: out =
// residue (KYSampler.Sample into a pool poly).  Up to two components of `batch` polys each in one launch.
struct NoiseLaunch {
    const u64 *x[2];
    u64 *out[2];
    const unsigned char *e[2];                     // device [batch][n]
    const u64 *plus[2];                            // nullptr: none
    long long x_stride[2], out_stride[2], plus_stride[2];
    int n, add;
    const LimbParams *lp;
};
hipError_t launch_bfv_noise(const NoiseLaunch &L, int comps, int limbs, int batch, hipStream_t stream);
inline LaunchVerdict launch_verdict(const NoiseLaunch &L, int comps, int limbs, int batch) {
    return launch_verdict(limbs <= 0 || batch <= 0 || comps <= 0, comps > 2 || L.n < 2 || (long long)comps * limbs > 65535);
}
// out = q - MRed(a, b): Neg(MulCoeffsMontgomery(crp, sk)) of skEncryptor.encrypt (bfv/encryptor.go:314-315, 326-327) in one pass; a zero
// product gives q, as Context.Neg does
struct NegMulLaunch {
    const u64 *a, *b;
    u64 *out;
    long long a_stride, b_stride, out_stride;      // between batch polys (0 = broadcast)
    int n;
    const LimbParams *lp;
};
hipError_t launch_bfv_negmul(const NegMulLaunch &L, int limbs, int batch, hipStream_t stream);
inline LaunchVerdict launch_verdict(const NegMulLaunch &L, int limbs, int batch) { return launch_verdict(limbs <= 0 || batch <= 0, L.n < 2); }

// ---- ckks.Encryptor (lr_ckks_encrypt.hip): the fast forms of ckks/encryptor.go around one forward transform ----
// the operands of that transform in one launch: `ternary` (0 or 1) polys from the two bit planes (as TernaryLaunch), then `noises` (0 .. 2)
// polys from the Gaussian samplers' bytes, part k of `batch` polys at out + k * part_stride.  A noise coefficient is the reference's
// residue (sign 1 -> c, sign 0 -> q - c) with the q of (0, sign 0) written as 0: the transform that follows reduces it to that anyway.
struct CkksExpandLaunch {
    const unsigned char *coeff_bits, *sign_bits;   // device [batch][n / 8]
    const unsigned char *e[2];                     // device [batch][n]
    u64 *out;
    long long out_stride, part_stride;
    int n, ternary, noises;
    LimbScalars one, minus_one;
    const LimbParams *lp;
};
hipError_t launch_ckks_expand(const CkksExpandLaunch &L, int limbs, int batch, hipStream_t stream);
inline LaunchVerdict launch_verdict(const CkksExpandLaunch &L, int limbs, int batch) {
    return launch_verdict(limbs <= 0 || batch <= 0 || L.ternary + L.noises <= 0,
                          L.n < 8 || limbs > kMaxLimbs || L.ternary < 0 || L.ternary > 1 || L.noises < 0 || L.noises > 2 || batch > 65535);
}
// pkEncryptor.encrypt, fast (ckks/encryptor.go:187-200, :234): out_k = CRed(MRed(u, pk_k) + e_k), out0 = CRed(out0 + pt); u, e0, e1 are
// the transformed polys of one expansion (poly stride r_stride)
struct CkksPkFastLaunch {
    const u64 *u, *e0, *e1, *pk0, *pk1, *pt;
    u64 *out0, *out1;
    long long r_stride, pk0_stride, pk1_stride, pt_stride, out0_stride, out1_stride;   // between batch polys (0 = broadcast)
    int n;
    const LimbParams *lp;
};
hipError_t launch_ckks_pk_fast(const CkksPkFastLaunch &L, int limbs, int batch, hipStream_t stream);
inline LaunchVerdict launch_verdict(const CkksPkFastLaunch &L, int limbs, int batch) { return launch_verdict(limbs <= 0 || batch <= 0, L.n < 2 || batch > 65535); }
// skEncryptor.encrypt, fast (ckks/encryptor.go:324-330, :359): out0 = CRed(CRed((q - MRed(crp, sk)) + e) + pt), out1 = crp
struct CkksSkFastLaunch {
    const u64 *crp, *sk, *e, *pt;
    u64 *out0, *out1;
    long long crp_stride, sk_stride, e_stride, pt_stride, out0_stride, out1_stride;
    int n;
    const LimbParams *lp;
};
hipError_t launch_ckks_sk_fast(const CkksSkFastLaunch &L, int limbs, int batch, hipStream_t stream);
inline LaunchVerdict launch_verdict(const CkksSkFastLaunch &L, int limbs, int batch) { return launch_verdict(limbs <= 0 || batch <= 0, L.n < 2 || batch > 65535); }

// ---- KeyGenerator (lr_keygen.hip): newSwitchingKey and GenPublicKey of ckks/keygen.go and bfv/keygen.go around one forward transform ----
constexpr int kKeygenKeysPerLaunch = 32;   // keys whose addresses and Galois elements travel in one launch's kernel arguments
// SwitchingKey.evakey as lr_ckks_switch_keys reads it: member m of the key at base + m * stride, 2 i = evakey[i][0], 2 i + 1 = evakey[i][1]
struct KeygenKeyRef {
    u64 *base;
    long long stride;
};
// skIn of `keys` keys over the rows of Q: out[k] = MRed(PermuteNTT(sk[k], gen[k]), MForm(P mod q)); gen = 1: no permutation
struct KeygenSkInLaunch {
    const u64 *sk;
    u64 *out;
    long long sk_stride, out_stride;               // between keys (sk: 0 = one secret key for all)
    u32 gen[kKeygenKeysPerLaunch];                 // Galois elements modulo 2 N, odd
    int n, logn;
    LimbScalars pmont;                             // MForm(P mod q) per limb of Q
    const LimbParams *lp;
};
hipError_t launch_keygen_skin(const KeygenSkInLaunch &L, int limbs, int keys, hipStream_t stream);
inline LaunchVerdict launch_verdict(const KeygenSkInLaunch &L, int limbs, int keys) {
    return launch_verdict(limbs <= 0 || keys <= 0,
                          L.n < 2 || L.logn < 1 || L.logn > 30 || (1 << L.logn) != L.n || limbs > kMaxLimbs || keys > kKeygenKeysPerLaunch);
}
// out[k] = P sk^(first + k + 2) over the rows of Q, k < keys: GenRelinKey's running product
struct KeygenPowersLaunch {
    const u64 *sk;
    u64 *out;
    long long out_stride;
    int n, first, keys;
    LimbScalars pmont;
    const LimbParams *lp;
};
hipError_t launch_keygen_powers(const KeygenPowersLaunch &L, int limbs, hipStream_t stream);
inline LaunchVerdict launch_verdict(const KeygenPowersLaunch &L, int limbs) { return launch_verdict(limbs <= 0 || L.keys <= 0, L.n < 2 || limbs > kMaxLimbs || L.first < 0); }
// evakey[i][0] = CRed(CRed(MForm(e) + [row in digit i] P skIn) + (q - MRed(evakey[i][1], skOut))) for `keys` keys x beta digits, every row of
// Q||P; e = the transformed noise of item k * beta + i
struct KeygenFinishLaunch {
    const u64 *e, *skin, *skout;
    long long e_stride, skin_stride, skout_stride; // e: between items; skin, skout: between keys (skout: 0 = shared)
    KeygenKeyRef key[kKeygenKeysPerLaunch];
    int n, nQ, alpha, beta;
    const LimbParams *lp;                          // of contextQP
};
hipError_t launch_keygen_finish(const KeygenFinishLaunch &L, int rows, int keys, hipStream_t stream);
inline LaunchVerdict launch_verdict(const KeygenFinishLaunch &L, int rows, int keys) {
    return launch_verdict(rows <= 0 || keys <= 0, L.n < 2 || rows > kMaxLimbs || keys > kKeygenKeysPerLaunch || L.beta < 1 || L.beta > kMaxLimbs ||
                                                      L.alpha < 1 || L.nQ < 1 || L.nQ > rows);
}
// pk0 = q - CRed(pk0 + MRed(sk, pk1)), pk0 holding NTT(e) on entry: GenPublicKey (ckks/keygen.go:144-148)
struct KeygenPkLaunch {
    const u64 *sk, *pk1;
    u64 *pk0;
    long long sk_stride, pk1_stride, pk0_stride;   // between batch polys (sk: 0 = broadcast)
    int n;
    const LimbParams *lp;
};
hipError_t launch_keygen_pk(const KeygenPkLaunch &L, int rows, int batch, hipStream_t stream);
inline LaunchVerdict launch_verdict(const KeygenPkLaunch &L, int rows, int batch) { return launch_verdict(rows <= 0 || batch <= 0, L.n < 2 || rows > kMaxLimbs || batch > 65535); }

// ---- dckks / dbfv collective key switching (lr_collective.hip): CKSProtocol, PCKSProtocol, AggregateShares, KeySwitch ----
constexpr int kFoldSharesPerLaunch = 32;   // shares whose addresses and strides travel in one launch's kernel arguments
// out = CRed(MRed(MRed(c1, CRed(sk_in + q - sk_out)), MForm(P mod q)) + e) over the rows of Q in the NTT domain: Sub, MulCoeffsMontgomery,
// MulScalarBigint and Add of genShareDelta (dckks/keyswitching.go:64-80) in one pass; e == nullptr: no addend (dbfv/keyswitching.go:76-90,
// whose noise arrives after the inverse transform)
struct CksShareLaunch {
    const u64 *c1, *sk_in, *sk_out, *e;
    u64 *out;
    long long c1_stride, sk_in_stride, sk_out_stride, e_stride, out_stride;   // between batch polys (keys: 0 = broadcast)
    int n;
    LimbScalars pmont;                                                         // MForm(P mod q) per limb of Q
    const LimbParams *lp;
};
hipError_t launch_cks_share(const CksShareLaunch &L, int limbs, int batch, hipStream_t stream);
inline LaunchVerdict launch_verdict(const CksShareLaunch &L, int limbs, int batch) { return launch_verdict(limbs <= 0 || batch <= 0, L.n < 2 || limbs > kMaxLimbs || batch > 65535); }
// out0 = CRed(out0 + MRed(c1, sk)): MulCoeffsMontgomeryAndAddLvl at the end of PCKSProtocol.GenShare (dckks/public_keyswitching.go:90)
struct PcksAddendLaunch {
    const u64 *c1, *sk;
    u64 *out0;
    long long c1_stride, sk_stride, out0_stride;
    int n;
    const LimbParams *lp;
};
hipError_t launch_pcks_addend(const PcksAddendLaunch &L, int limbs, int batch, hipStream_t stream);
inline LaunchVerdict launch_verdict(const PcksAddendLaunch &L, int limbs, int batch) { return launch_verdict(limbs <= 0 || batch <= 0, L.n < 2 || limbs > kMaxLimbs || batch > 65535); }
// acc = share[0]; acc = CRed(acc + share[k]) for k = 1 .. count - 1 in this order; out = base ? CRed(base + acc) : acc.  Element-wise: out
// may be base or any share as a whole poly.
struct FoldShareRef {
    const u64 *base;
    long long stride;
};
struct FoldLaunch {
    FoldShareRef share[kFoldSharesPerLaunch];
    int count;
    const u64 *base;                                                           // nullptr: none
    u64 *out;
    long long base_stride, out_stride;
    int n;
    const LimbParams *lp;
};
hipError_t launch_fold(const FoldLaunch &L, int limbs, int batch, hipStream_t stream);
inline LaunchVerdict launch_verdict(const FoldLaunch &L, int limbs, int batch) {
    return launch_verdict(limbs <= 0 || batch <= 0, L.n < 2 || limbs > kMaxLimbs || batch > 65535 || L.count < 1 || L.count > kFoldSharesPerLaunch);
}

// ---- dckks / dbfv collective key setup (lr_setup.hip): CKGProtocol, RKGProtocol, RKGProtocolNaive, RTGProtocol ----
constexpr int kSetupPartiesPerLaunch = 32;   // parties (RTG: Galois elements) whose share addresses travel in one launch's kernel arguments
// CKGProtocol.GenShare (dbfv/publickey_gen.go:54-57): share = CRed(share + (q - MRed(sk, crs))), share holding NTT(e) on entry
struct SetupCkgLaunch {
    const u64 *sk, *crs;
    u64 *share;
    long long sk_stride, crs_stride, share_stride;   // between parties (sk, crs: 0 = shared)
    int n;
    const LimbParams *lp;
};
hipError_t launch_setup_ckg(const SetupCkgLaunch &L, int rows, int batch, hipStream_t stream);
inline LaunchVerdict launch_verdict(const SetupCkgLaunch &L, int rows, int batch) { return launch_verdict(rows <= 0 || batch <= 0, L.n < 2 || rows > kMaxLimbs || batch > 65535); }
// what the share kernels of RKG, the naive RKG and RTG read: z = party * beta + digit on blockIdx.z, every row of Q||P.  e = the
// transformed noise, `per` polys per z (item z * per + c); t = the transformed ternary of item z; out[party] = the party's share,
// member digit (a share of polys) or members 2 digit and 2 digit + 1 (a share of pairs).  Digit i owns rows i alpha .. min((i + 1)
// alpha, nQ) - 1; there skP = InvMForm(MRed(sk, MForm(P mod q))) is added (dbfv/relinkey_gen.go:223-250).
struct SetupShareLaunch {
    const u64 *e, *t;
    long long e_stride, t_stride;
    const u64 *sk, *u;
    long long sk_stride, u_stride;                 // between parties (0 = one key for the call)
    const u64 *crp;                                // member digit: crp[digit]
    long long crp_stride;
    const u64 *in;                                 // the aggregate of the round before: member digit, or members 2 digit, 2 digit + 1
    long long in_stride;
    const u64 *pk0, *pk1;                          // the collective public key (naive RKG)
    KeygenKeyRef out[kSetupPartiesPerLaunch];
    u32 gen[kSetupPartiesPerLaunch];               // RTG: Galois elements modulo 2 N, odd
    int n, logn, nQ, alpha, beta;
    int quirk;                                     // naive round one, dckks: e[i][1] is the noise of [i][0], [i][1] has none
    LimbScalars pmont;                             // MForm(P mod q) per limb of Q
    const LimbParams *lp;                          // of contextQP
};
enum SetupShareKind { kSetupRkg1, kSetupRkg2, kSetupRkg3, kSetupNaive1, kSetupNaive2, kSetupRtg };
hipError_t launch_setup_share(int kind, const SetupShareLaunch &L, int rows, int parties, hipStream_t stream);
// (the kind is the launcher's own switch: an unknown one is refused there)
inline LaunchVerdict launch_verdict(const SetupShareLaunch &L, int rows, int parties) {
    return launch_verdict(rows <= 0 || parties <= 0, L.n < 2 || L.logn < 1 || L.logn > 30 || (1 << L.logn) != L.n || rows > kMaxLimbs ||
                                                         parties > kSetupPartiesPerLaunch || L.beta < 1 || L.beta > kMaxLimbs || L.alpha < 1 ||
                                                         L.nQ < 1 || L.nQ > rows);
}
// the finalize steps over the beta digits of one key image (member 2 i = [i][0], 2 i + 1 = [i][1]), z = digit:
//   RKG    (dbfv/relinkey_gen.go:343-354): evk[i][0] = MForm(CRed(round2[i][0] + round3[i])), evk[i][1] = MForm(round2[i][1])
//   naive  (dbfv/relinkey_gen_naive.go:187-200): the same without a round3
//   RTG    (dbfv/rotkey_gen.go:205-214): key[i][0] = share[i], key[i][1] = MForm(crp[i])
// Element-wise: evk may be round2 as a whole poly.
struct SetupKeyLaunch {
    const u64 *pairs;                              // round2: members 2 i, 2 i + 1; nullptr: RTG
    const u64 *polys;                              // round3, or RTG's share; nullptr: naive
    const u64 *crp;                                // RTG only
    u64 *key;
    long long pairs_stride, polys_stride, crp_stride, key_stride;
    int n;
    const LimbParams *lp;
};
hipError_t launch_setup_key(const SetupKeyLaunch &L, int rows, int beta, hipStream_t stream);
inline LaunchVerdict launch_verdict(const SetupKeyLaunch &L, int rows, int beta) {
    return launch_verdict(rows <= 0 || beta <= 0, L.n < 2 || rows > kMaxLimbs || beta > kMaxLimbs || (!L.pairs && (!L.polys || !L.crp)));
}

// ---- dckks / dbfv Refresh (lr_refresh.hip): RefreshProtocol.GenShares, Recode, Recrypt, Finalize ----
constexpr int kCkksCrtMaxWords = 32;            // 64-bit words of the largest Q the CKKS decoder's CRT takes (2048 bits), and of a Refresh mask
// out[b][i][j] = big.Int.Mod(mask[b][j], q_i) for i < limbs: SetCoefficientsBigint(Lvl) (ring/ring_context.go:343-367) of a signed integer
// in two's complement on `words` little-endian 64-bit words, word planes [batch][words][N]
struct RefreshMaskLaunch {
    const u64 *mask;
    u64 *out;
    long long out_stride;
    int n, words;
    LimbScalars two64;                 // 2^64 mod q_i
    const LimbParams *lp;
};
hipError_t launch_refresh_mask(const RefreshMaskLaunch &L, int limbs, int batch, hipStream_t stream);
inline LaunchVerdict launch_verdict(const RefreshMaskLaunch &L, int limbs, int batch) {
    return launch_verdict(limbs <= 0 || batch <= 0, L.n < 2 || L.words < 1 || L.words > kCkksCrtMaxWords || limbs > kMaxLimbs || batch > 65535);
}
// dckks GenShares :78-92 on one row of Q, NTT domain.  Rows below dec_limbs: dec = CRed(CRed(mask + MRed(sk, c1)) + e0); every row:
// rec = q - CRed(CRed(mask + MRed(sk, crs)) + e1)
struct RefreshCkksShareLaunch {
    const u64 *mask, *e0, *e1, *sk, *c1, *crs;
    u64 *dec, *rec;
    long long r_stride, sk_stride, c1_stride, crs_stride, dec_stride, rec_stride;   // r_stride: of mask, e0 and e1 (sk: 0 = broadcast)
    int n, dec_limbs;
    const LimbParams *lp;
};
hipError_t launch_refresh_ckks_share(const RefreshCkksShareLaunch &L, int limbs, int batch, hipStream_t stream);
inline LaunchVerdict launch_verdict(const RefreshCkksShareLaunch &L, int limbs, int batch) {
    return launch_verdict(limbs <= 0 || batch <= 0, L.n < 2 || limbs > kMaxLimbs || L.dec_limbs < 1 || L.dec_limbs > limbs || batch > 65535);
}
// dckks Recode :114-136 per coefficient, coefficient domain: v = the CRT of rows 0 .. ls of `in` in [0, Q_ls) as mixed-radix digits (Garner),
// v >= Q_ls >> 1 => v -= Q_ls, out[i] = v mod q_i (Euclidean) for rows row0 .. limbs - 1 of `out`
struct RefreshRecodeLaunch {
    const u64 *in;
    u64 *out;
    long long in_stride, out_stride;
    int n, ls, row0, limbs;
    const u64 *qmod;                   // [limbs][limbs]: q_m mod q_k at [k][m]
    const u64 *ginv;                   // [limbs]: (q_0 ... q_(k-1))^-1 mod q_k
    const u64 *hdig;                   // [ls + 1]: the mixed-radix digits of Q_ls >> 1
    const u64 *qls;                    // [limbs]: Q_ls mod q_i
    const LimbParams *lp;
};
hipError_t launch_refresh_recode(const RefreshRecodeLaunch &L, int batch, hipStream_t stream);
inline LaunchVerdict launch_verdict(const RefreshRecodeLaunch &L, int batch) {
    return launch_verdict(batch <= 0 || L.row0 >= L.limbs, L.n < 2 || L.limbs > kMaxLimbs || L.ls < 0 || L.ls >= L.limbs || L.row0 < 0 || batch > 65535);
}
// dbfv GenShares :117-122 and :141-142 on one row of Q||P, NTT domain, in place: rows of Q: a = MRed(MRed(sk, a), MForm(P mod q));
// every row: b = q - MRed(sk, b) (Neg: a zero becomes q)
struct RefreshBfvProductLaunch {
    const u64 *sk;
    u64 *a, *b;
    long long sk_stride, stride;
    int n, nQ;
    LimbScalars pmont;
    const LimbParams *lp;              // of contextQP
};
hipError_t launch_refresh_bfv_product(const RefreshBfvProductLaunch &L, int rows, int batch, hipStream_t stream);
inline LaunchVerdict launch_verdict(const RefreshBfvProductLaunch &L, int rows, int batch) {
    return launch_verdict(rows <= 0 || batch <= 0, L.n < 2 || rows > kMaxLimbs || L.nQ < 1 || L.nQ > rows || batch > 65535);
}
// dbfv lift :199-205 and what follows it: m = MRed(row, deltaMont_i); dec = CRed(dec + m) and, with rec, rec = CRed(rec + q - m) (GenShares
// :153-159); plus: dec = CRed(m + plus) (Recode's lift and Recrypt's Add, :178-185)
struct RefreshBfvLiftLaunch {
    const u64 *row, *plus;             // row: [batch][N]
    u64 *dec, *rec;
    long long plus_stride, dec_stride, rec_stride;
    int n;
    const u64 *delta_mont;             // [limbs]
    const LimbParams *lp;
};
hipError_t launch_refresh_bfv_lift(const RefreshBfvLiftLaunch &L, int limbs, int batch, hipStream_t stream);
inline LaunchVerdict launch_verdict(const RefreshBfvLiftLaunch &L, int limbs, int batch) {
    return launch_verdict(limbs <= 0 || batch <= 0, L.n < 2 || limbs > kMaxLimbs || batch > 65535 || !L.dec || (L.plus == nullptr) == (L.rec == nullptr));
}

// ---- ckks.Encoder (lr_ckks_encode.hip): Encode / Decode of ckks/encoder.go for a batch of plaintexts ----
struct Cplx { double re, im; };                 // a complex128 as Go lays it out
constexpr int kCkksFusedMaxLogSlots = 13;       // the fused kernels hold 16 * slots bytes in one CU's LDS: 128 KiB of the 160
constexpr int kCkksOneKernelBatch = 256;        // fused Encode as ONE kernel from this batch on: a workgroup per CU of the MI355X (below)
constexpr int kCkksTileMaxLog = 11;             // the tiled route's LDS tile, at most 2^11 slots (32 KiB)
// NewEncoder's tables (ckks/encoder.go:37-53): roots[0 .. m] with m = 2 N, rotGroup[j] = 5^j mod m for j < N / 2
struct CkksEncTables {
    const Cplx *roots;     // [2 N + 1]
    const u32 *rot;        // [N / 2]
    int n, logn;
};
// scaleUpVecExact's target (ckks/utils.go:51-98): limbs 0 .. limbs - 1 of a plaintext poly, coefficient domain
struct CkksScaleUp {
    u64 *out;
    long long out_stride;
    int limbs;
    const LimbParams *lp;  // of contextQ
    double scale;
};
// the tile of the tiled route for 2^logslots slots: a quarter of the slots, so that streaming stages run at every size, up to the LDS tile
inline int ckks_tile_log(int logslots) { return logslots < 2 ? 0 : (logslots - 2 < kCkksTileMaxLog ? logslots - 2 : kCkksTileMaxLog); }
// fused Encode, one workgroup per plaintext: values [batch][slots] -> invfft in LDS -> scale-up into the limbs; slots <= 2^13.  A workgroup
// writes all (level + 1) N words of its plaintext, so the host uses it once the batch fills the chip (kCkksOneKernelBatch); a smaller batch
// runs invfft in LDS through launch_ckks_dif_tile with the whole slot vector as the tile, then launch_ckks_scale_up over the whole grid
hipError_t launch_ckks_encode_fused(const CkksEncTables &tab, const Cplx *values, int logslots, const CkksScaleUp &S, int batch, hipStream_t stream);
// tiled Encode: the stage len = 2^loglen of invfftlazy (:170-190) over [batch][slots] in global memory (src == dst allowed) ...
hipError_t launch_ckks_dif_stage(const CkksEncTables &tab, const Cplx *src, Cplx *dst, int logslots, int loglen, int batch, hipStream_t stream);
// ... the stages len = 2^logtile .. 2 in LDS, one tile per workgroup ...
hipError_t launch_ckks_dif_tile(const CkksEncTables &tab, const Cplx *src, Cplx *dst, int logslots, int logtile, int batch, hipStream_t stream);
// ... and the bit reversal, the division by slots and the scale-up from the stages' output
hipError_t launch_ckks_scale_up(const CkksEncTables &tab, const Cplx *src, int logslots, const CkksScaleUp &S, int batch, hipStream_t stream);
// Decode's coefficients (:122-152): CRT of limbs 0 .. limbs - 1 at the used coefficients, centred, to double exactly as
// big.Float.SetInt(..).Float64() rounds, divided by scale; dbuf = [batch][2 slots] (real parts, then imaginary parts)
struct CkksCrt {
    const u64 *pool;       // [batch][limbs][N], coefficient domain, canonical residues
    long long pool_stride;
    int limbs, words;      // words of Q_level
    const LimbParams *lp;
    const u64 *qhat;       // [limbs][qhat_stride]: Q_level / q_i, little-endian words
    long long qhat_stride;
    const u64 *inv;        // [limbs]: (Q_level / q_i)^-1 mod q_i
    const u64 *Q, *Qhalf;  // [words]: Q_level and Q_level >> 1
    double scale;
};
hipError_t launch_ckks_crt_to_double(const CkksEncTables &tab, const CkksCrt &P, int logslots, double *dbuf, int batch, hipStream_t stream);
// fft (:204-226): the bit reversal folded into the load and the stages len = 2 .. 2^logtile in LDS; logtile == logslots is the fused Decode
hipError_t launch_ckks_dit_tile(const CkksEncTables &tab, const double *dbuf, Cplx *dst, int logslots, int logtile, int batch, hipStream_t stream);
// the stage len = 2^loglen over [batch][slots] in global memory (src == dst allowed)
hipError_t launch_ckks_dit_stage(const CkksEncTables &tab, const Cplx *src, Cplx *dst, int logslots, int loglen, int batch, hipStream_t stream);

// ---- basis extension (lr_bext.hip) ----
struct ExtTables {        // device pointers; modupParams of ring_basis_extension.go:19-37
    int nQ, nP;
    const u64 *Q;         // [nQ]
    const u64 *mredQ;     // [nQ]
    const u64 *qib_mont;  // [nQ]
    const u64 *P;         // [nP]
    const u64 *mredP;     // [nP]
    const u64 *bredP_hi;  // [nP]
    const u64 *qispj_mont;// [nQ][nP]
    const u64 *qpj_inv;   // [nP][nQ+1]
    // the same (Q/q_i) mod p_j out of Montgomery form, with the Shoup companion floor(c * 2^64 / p_j): the
    // products y_i * c accumulate lazily and are reduced once, to the same canonical residue
    const ulonglong2 *qispj_shoup;  // [nQ][nP] {c, companion}
    const double *Qrcp;   // [nQ] RN(1 / float64(q_i)): div_by_const
    int fast_div_ok;      // every float64(q_i) satisfies div_by_const's precondition (significand not all ones, q_i >= 2): checked on the
                          // host at creation; 0 sends every extension of this table through the reference-shaped kernel and its IEEE division
    int lazy_terms;       // how many [0,4p) terms, each with one p of the correction v * qpjInv[1], fit in 64 bits
    int exact_terms;      // the same for [0,2p) terms
    int word_barrett;     // every p_j > 2^32: floor(2^64 / p_j) fits one word (ext_sum_kernel's final reduction)
    int wide_ok;          // how many input terms keep n * max q_i below 2^64 (ext_wide_kernel: one Montgomery reduction per group)
    // inputs that are the LAZY outputs of the inverse sub-block kernels (the two halves U, V of a limb before its last Gentleman-Sande
    // stage and the scaling): qib_mont[i] * N^-1 and qib_mont[i] * psi_inv[1] * N^-1 mod q_i, so that MRed(U + V, .) and
    // MRed(U + bound - V, .) are the y_i of the finished coefficients j and j + N/2 -- the last inverse stage costs the extension one
    // addition per coefficient instead of a pass over the rows (ExtLaunch::inv_top, top-stage variant of the sum-form kernel only);
    // null where the table was not given a context (set_inverse_top)
    const u64 *invtop0, *invtop1;
};

constexpr int kExtSegments = 3;   // key-switch digits: rows below the digit, rows above it, the special primes

struct ExtSegment {       // rows [limb0, limb0+count) of `out` receive table columns [col0, col0+count)
    u64 *out;
    long long stride;     // u64 elements between batch polys
    int limb0, col0, count;
    // top-stage variant (N = 2^16 key switch, ext_sum_kernel<.., true>): forward twiddle table of the context that owns the segment's
    // output moduli ([L][N] entries {w, floor(w 2^64 / q)}) and the modulus index of the segment's first row; nullptr = plain extension
    const Twiddle *top_tw;
    int top_mod0;
    // epilogue on the canonical extension value e of a row (target modulus p, table column col), plain (non-top) kernels only:
    //   1: out = CRed(MRed(x + (p - e), c[col]) + s[col])   x = the row of `epi_x` at the output's position: the subtract-multiply of a
    //      ModDown (ring_basis_extension.go:237-239) with the scalar addition that follows it in bfv/evaluator.go:457
    //   2: out = MRed(CRed(e + (p - s[col])), c[col])          bfv/evaluator.go:459,462 (SubScalarBigint, MulScalar)
    int epi_mode;               // 0 = none
    const u64 *epi_x;
    long long epi_x_stride;
    // mode 1 only, optional: x = CRed(x + x2) first -- the Gaussian residues SampleAndAdd adds to the Q rows in front of the ModDown of
    // pkEncryptor.encrypt (ckks/encryptor.go:218-226), read at the output's position like x
    const u64 *epi_x2;
    long long epi_x2_stride;
    const u64 *epi_c, *epi_s;   // device arrays over the table columns (epi_s == nullptr: zeros)
};

struct ExtLaunch {
    ExtTables t;
    const u64 *in;
    long long in_stride;
    int in_limb0;
    int n;
    ExtSegment seg[kExtSegments];   // unused segments have count == 0
    int inv_top;                    // 1: the input rows are lazy inverse sub-block outputs (ExtTables::invtop0 / invtop1)
};

constexpr int kExtGroupMax = 9;    // extensions per grouped launch (the digits of one key switch: beta = 9 at PN16QP1761)
struct ExtGroupLaunch {
    ExtLaunch L[kExtGroupMax];
};

#if defined(__HIPCC__)
// Tables that no kernel writes, read at wave-uniform addresses: through the constant address space, so that the
// compiler keeps using scalar loads after the kernel has started storing (it cannot prove that the stores do not
// alias a plain global pointer and falls back to one vector load round trip per use).
typedef const unsigned long __attribute__((address_space(4))) lr_const_u64;
__device__ __forceinline__ unsigned long ld_const(const unsigned long *p) { return *(lr_const_u64 *)(unsigned long)p; }
__device__ __forceinline__ ulonglong2 ld_const(const ulonglong2 *p) {
    lr_const_u64 *q = (lr_const_u64 *)(unsigned long)p;
    return make_ulonglong2(q[0], q[1]);
}

// streaming access to poly data (each element is read or written once per launch): the `nt` cache policy keeps
// it from displacing the twiddle / key tables in L2 and the Infinity Cache
typedef unsigned long long lr_u64x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ ulonglong2 ld_stream(const ulonglong2 *p) {
    const lr_u64x2 v = __builtin_nontemporal_load(reinterpret_cast<const lr_u64x2 *>(p));
    return make_ulonglong2(v.x, v.y);
}
__device__ __forceinline__ unsigned long ld_stream(const unsigned long *p) { return __builtin_nontemporal_load(p); }
__device__ __forceinline__ void st_stream(unsigned long *p, unsigned long v) { __builtin_nontemporal_store(v, p); }
__device__ __forceinline__ void st_stream(ulonglong2 *p, ulonglong2 v) {
    lr_u64x2 t;
    t.x = v.x;
    t.y = v.y;
    __builtin_nontemporal_store(t, reinterpret_cast<lr_u64x2 *>(p));
}

// The launch every launcher ends on: drop stale (non-sticky) errors of unrelated earlier calls, launch, and return this launch's own error.
template <class Kernel, class... Args>
inline hipError_t launch_kernel(Kernel kernel, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t stream, const Args &...args) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(kernel, grid, block, lds_bytes, stream, args...);
    return hipGetLastError();
}
#endif

// host launchers (defined next to their kernels)
// mode: lazy-correction cadence of the forward butterflies (lr_ntt.hip): 0 = q < 2^61, 1 = q <= 2^60, 2 = q < 2^57
hipError_t launch_ntt(const NttLaunch &a, int logn, bool inverse, int mode, hipStream_t stream);
// hand-scheduled assembly forward NTT (lr_asm.cpp); N = 2^14 / 2^15, lazy mode 1 only
bool ntt_asm_available(int logn);
// kernel_name (optional, >= 32 bytes): receives the name of the code object that was launched
// stagger: Options::stagger (kilo-clocks per step; 0 = off, -1 = the launcher's default for the kernel)
hipError_t launch_ntt_asm(const NttLaunch &a, int logn, int inverse, int variant, hipStream_t stream, bool wide14 = false,
                          char *kernel_name = nullptr, bool timeline = false, int stagger = -1, int persist = 0, bool pad_grid = true);
hipError_t launch_ntt_asm16(const NttLaunch &a, int inverse, char kind, int variant, hipStream_t stream, char *kernel_name = nullptr,
                            int stagger = -1, int full_logn = 16);
// N = 2^16 helpers (lr_ntt.hip): the streaming stage over bit 15, and whether no input row of a launch is an output row
hipError_t launch_ntt_top(const NttLaunch &a, int inverse, hipStream_t stream, int logn = 16);
// the rescale's three streaming passes between the lazy inverse sub-blocks of the last limb and the forward sub-blocks of the targets (lr_ntt.hip)
hipError_t launch_rescale_mid(const NttLaunch &a, const Twiddle *tw_inv, int last_mod, u64 phalf, int logn, hipStream_t stream);
// no input row of the launch is an output row (host arithmetic on the launch's addressing; the dispatcher asks before anything is launched)
inline bool ntt_rows_disjoint(const NttLaunch &a, int logn) {
    const long long n_full = 1ll << logn;
    const long long last = (long long)(a.n_items - 1 + (a.hole > 0 ? a.hole : 0));
    const u64 *in_lo = a.in + (long long)a.in_limb0 * n_full;
    const u64 *in_hi = a.in + (long long)(a.batch - 1) * a.in_poly_stride + ((long long)a.in_limb0 + last * a.in_limb_step + 1) * n_full;
    const u64 *out_lo = a.out + (long long)a.out_limb0 * n_full;
    const u64 *out_hi = a.out + (long long)(a.batch - 1) * a.out_poly_stride + ((long long)a.out_limb0 + last * a.out_limb_step + 1) * n_full;
    const bool positive = a.in_poly_stride >= 0 && a.out_poly_stride >= 0 && a.in_limb_step >= 0 && a.out_limb_step >= 0;
    if (!positive) return false;
    if (in_hi <= out_lo || out_hi <= in_lo) return true;
    // rows of the same polys (Rescale: the last limb's row into the rows below it): compare the row sets inside one poly
    if (a.in != a.out || a.in_poly_stride != a.out_poly_stride || a.n_items > 256) return false;
    const long long top_row = std::max((long long)a.in_limb0 + last * a.in_limb_step, (long long)a.out_limb0 + last * a.out_limb_step);
    if (a.batch > 1 && a.in_poly_stride < (top_row + 1) * n_full) return false;
    for (long long i = 0; i <= last; ++i)
        for (long long j = 0; j <= last; ++j)
            if (a.in_limb0 + i * a.in_limb_step == a.out_limb0 + j * a.out_limb_step) return false;
    return true;
}
hipError_t launch_ewise(int op, const EwiseLaunch &L, int limbs, int batch, hipStream_t stream);
hipError_t launch_submul(const SubMulLaunch &L, int limbs, int batch, hipStream_t stream);
hipError_t launch_rowadd(const RowAddLaunch &L, int rows, int batch, hipStream_t stream);
hipError_t launch_half_scalar(const HalfScalarLaunch &L, int limbs, int batch, hipStream_t stream);
hipError_t launch_ext(const ExtLaunch &L, int n_in, int batch, hipStream_t stream);
// `count` extensions of the same shape (n_in input limbs each) as one launch; hipErrorNotSupported when the shape has no grouped form
hipError_t launch_ext_group(const ExtLaunch *Ls, int count, int n_in, int batch, hipStream_t stream);
bool ext_top_supported(const ExtTables &t, int n_in, int n);
bool ext_epilogue_supported(const ExtTables &t, int n_in, int n);
hipError_t launch_div_selftest(u64 seed, int blocks, int per_thread, unsigned long long *d_mismatches, hipStream_t stream);

}  // namespace lr
