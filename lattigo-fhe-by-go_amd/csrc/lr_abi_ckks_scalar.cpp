// lr_abi_ckks_scalar.cpp -- C ABI: the scalar side of ckks.Evaluator's calls, host only (no context, no device): the levels, scales and
// per-limb words that the element side (lr_abi_ckks_eval.cpp) takes as arguments, and what the reference panics on.
//   lr_ckks_lincomb_constants      res = c0 + sum_k c_k ct_k, the leaf of the reference's polynomial evaluation (evaluatePolyFromPowerBasis,
//                                  ckks/polynomial_evaluation.go:142-159: one AddConst and a chain of MultByConstAndAdd)
//   lr_ckks_combine_constants      out = a (+|-) b at any scale, level and degree (evaluateInPlace, ckks/evaluator.go:153-342): which operand
//                                  is multiplied and by which words, the level, scale and degree of the result
//   lr_ckks_power_basis_schedule   the power basis C[n] = C[ceil(n/2)] * C[n >> 1] (computePowerBasis, ckks/polynomial_evaluation.go:76-93)
//                                  and C[n] = 2 C[a] C[b] - C[a - b] (computePowerBasisCheby, ckks/chebyshev_evaluation.go:60-101), and with
//                                  them PowerOf2 (ckks/algorithms.go:9-31), which is computePowerBasis(2^k): which products, in the
//                                  reference's order, and per product the level, the Rescale loop's trip count, the scale and the words of
//                                  the Chebyshev tail.  Sub's words come from lr_ckks_combine_constants, AddConst's from lr_ckks_scalar.hpp.
#include "lr_ckks_scalar.hpp"

namespace lr_host {
namespace {
using namespace ckks_scalar;

const char *const kLincomb = "CKKS linear combination constants: ";
const char *const kCombine = "CKKS combine constants: ";
const char *const kSchedule = "CKKS power basis schedule: ";

int refuse(const char *who, int code, const char *what) { return fail(code, std::string(who) + what); }

// the domain of the moduli, and of the root words where a call has them
int check_moduli(const char *who, const u64 *moduli, int n_moduli, const u64 *ntt_psi1 = nullptr) {
    for (int i = 0; i < n_moduli; ++i) {
        if (moduli[i] < 3 || !(moduli[i] & 1) || (moduli[i] >> 61)) return refuse(who, LR_ERR_ARG, "a modulus is even, below 3 or not below 2^61");
        if (ntt_psi1 && ntt_psi1[i] >= moduli[i]) return refuse(who, LR_ERR_ARG, "a root word is not below its modulus");
    }
    return LR_OK;
}

// the recursion of :78-92 / :70-99: a, then b, each only when not yet present (c is 0 or 1 and C[1] is always present)
struct Recursion {
    std::map<u32, int> at;               // n -> its product
    std::vector<u32> order;
    void want(u32 n) {
        if (n == 1 || at.count(n)) return;
        want((n + 1) >> 1);
        want(n >> 1);
        at[n] = (int)order.size();
        order.push_back(n);
    }
};

}  // namespace
}  // namespace lr_host

extern "C" int lr_ckks_lincomb_constants(const uint64_t *moduli, const uint64_t *ntt_psi1, int n_moduli, double default_scale, int res_level,
                                         double res_scale, int has_const, double c0_re, double c0_im, int n_terms, const double *term_re,
                                         const double *term_im, const double *term_scale, const int *term_level, int *level_after,
                                         double *scale_after, uint64_t *add_lo, uint64_t *add_hi, uint8_t *has_pre, uint64_t *pre, uint64_t *lo,
                                         uint64_t *hi) {
    return guarded([&]() -> int {
    const auto refuse_const = [](const char *what) { return refuse(kLincomb, LR_ERR_ARG, what); };
    if (!moduli || !ntt_psi1 || !level_after || !scale_after) return refuse_const("null argument");
    if (has_const && (!add_lo || !add_hi)) return refuse_const("null argument");
    if (n_terms > 0 && (!term_re || !term_im || !term_scale || !term_level || !has_pre || !pre || !lo || !hi)) return refuse_const("null argument");
    if (n_moduli < 1 || n_terms < 0 || res_level < 0 || res_level >= n_moduli) return refuse_const("a count or a level is out of range");
    for (int k = 0; k < n_terms; ++k)
        if (term_level[k] < 0 || term_level[k] >= n_moduli) return refuse_const("a count or a level is out of range");
    LR_TRY(check_moduli(kLincomb, moduli, n_moduli, ntt_psi1));
    if (!scale_ok(default_scale) || !scale_ok(res_scale)) return refuse_const("a scale is not finite and positive");
    for (int k = 0; k < n_terms; ++k)
        if (!scale_ok(term_scale[k])) return refuse_const("a scale is not finite and positive");
    if (has_const && (!magnitude_ok(c0_re) || !magnitude_ok(c0_im))) return refuse_const("a constant is not finite and below 2^63 in magnitude");
    for (int k = 0; k < n_terms; ++k)
        if (!magnitude_ok(term_re[k]) || !magnitude_ok(term_im[k])) return refuse_const("a constant is not finite and below 2^63 in magnitude");

    // DropLevel (:457-460) only lowers the receiver's level and the limbs above the final level are dropped: the words of limbs
    // 0 .. level_after are what remains of every step, whatever level the step ran at
    int level = res_level;
    for (int k = 0; k < n_terms; ++k) level = std::min(level, term_level[k]);
    const int L1 = level + 1;
    std::vector<Limb> limb((size_t)L1);
    for (int i = 0; i < L1; ++i) limb[i] = limb_of(moduli[i], ntt_psi1[i]);
    const auto product_ok = [](double re, double im, double scale) { return std::isfinite(scale * re) && std::isfinite(scale * im); };
    const char *const kRatio = "a scale ratio is not below 2^63";
    const char *const kProduct = "a constant times its scale is not finite";

    std::vector<u64> v_add_lo((size_t)L1), v_add_hi((size_t)L1), v_pre((size_t)n_terms * L1), v_lo((size_t)n_terms * L1), v_hi((size_t)n_terms * L1);
    std::vector<uint8_t> v_has_pre((size_t)n_terms, 0);
    double scale_out = res_scale;
    if (has_const) {     // AddConst(res, c0, res), :373-444: ct0 is the receiver, its scale stays
        if (!product_ok(c0_re, c0_im, scale_out)) return refuse_const(kProduct);
        for (int i = 0; i < L1; ++i) half_constants(c0_re, c0_im, scale_out, limb[i], &v_add_lo[i], &v_add_hi[i]);
    }
    for (int k = 0; k < n_terms; ++k) {     // MultByConstAndAdd(ct_k, c_k, res), :451-608
        const double re = term_re[k], im = term_im[k], ct_scale = term_scale[k];
        double scale = 1;
        if (has_fraction(re)) scale = default_scale;
        if (has_fraction(im)) scale = default_scale;
        u64 *pre_k = &v_pre[(size_t)k * L1];
        if (scale != 1) {
            if (scale_out < ct_scale * default_scale) {                                                 // :526
                const double ratio = (default_scale * ct_scale) / scale_out;
                if (!(ratio >= 0 && ratio < kTwo63)) return refuse_const(kRatio);
                if ((u64)ratio != 0) {                                                                  // :528
                    // MultByConst(ctOut, uint64(ratio), ctOut), :530: an integer constant, scale 1 (:669-671)
                    v_has_pre[k] = 1;
                    for (int i = 0; i < L1; ++i) pre_k[i] = integer_multiplier_word(ratio, limb[i]);
                }
                scale_out = default_scale * ct_scale;                                                   // :534
            } else if (scale_out > ct_scale * default_scale) {                                          // :538
                scale = scale_out / ct_scale;
            }
        } else {
            if (scale_out > ct_scale) {                                                                 // :546
                scale = scale_out / ct_scale;
            } else if (ct_scale > scale_out) {                                                          // :550
                const double ratio = ct_scale / scale_out;
                if (!(ratio >= 0 && ratio < kTwo63)) return refuse_const(kRatio);
                if ((u64)ratio != 0) {                                                                  // :552
                    // MultByConst(ctOut, ratio, ctOut), :553: a float64 constant -- with a fractional part it is scaled by the default
                    // scale (:656-667), and the scale that call sets (:733) is overwritten at :556.  The lines as they stand.
                    const double scale_m = has_fraction(ratio) ? default_scale : 1;
                    if (!product_ok(ratio, 0, scale_m)) return refuse_const(kProduct);
                    v_has_pre[k] = 1;
                    for (int i = 0; i < L1; ++i) {
                        u64 unused;
                        half_constants_mform(ratio, 0, scale_m, limb[i], &pre_k[i], &unused);
                    }
                }
                scale_out = ct_scale;                                                                   // :556
            }
        }
        if (!product_ok(re, im, scale)) return refuse_const(kProduct);
        for (int i = 0; i < L1; ++i) half_constants_mform(re, im, scale, limb[i], &v_lo[(size_t)k * L1 + i], &v_hi[(size_t)k * L1 + i]);
    }
    // nothing was written so far
    *level_after = level;
    *scale_after = scale_out;
    if (has_const) {
        std::copy(v_add_lo.begin(), v_add_lo.end(), add_lo);
        std::copy(v_add_hi.begin(), v_add_hi.end(), add_hi);
    }
    if (n_terms > 0) {
        std::copy(v_has_pre.begin(), v_has_pre.end(), has_pre);
        std::copy(v_pre.begin(), v_pre.end(), pre);
        std::copy(v_lo.begin(), v_lo.end(), lo);
        std::copy(v_hi.begin(), v_hi.end(), hi);
    }
    return LR_OK;
    });
}

extern "C" int lr_ckks_combine_constants(const uint64_t *moduli, int n_moduli, int op, int a_degree, int a_level, double a_scale, int b_degree,
                                         int b_level, double b_scale, int out_degree, int out_level, double out_scale, int receiver,
                                         int *level_after, double *scale_after, int *degree_after, int *mult_side, uint64_t *mult) {
    return guarded([&]() -> int {
    const auto refuse_const = [](int code, const char *what) { return refuse(kCombine, code, what); };
    if (!moduli || !level_after || !scale_after || !degree_after || !mult_side || !mult) return refuse_const(LR_ERR_ARG, "null argument");
    const auto degree_ok = [](int d) { return d >= 0 && d <= 2; };
    const auto level_ok = [&](int l) { return l >= 0 && l < n_moduli; };
    if (n_moduli < 1 || op < LR_ADD || op > LR_SUB_NOMOD || receiver < LR_COMBINE_OUT_NEW || receiver > LR_COMBINE_OUT_BOTH || !degree_ok(a_degree) ||
        !degree_ok(b_degree) || !degree_ok(out_degree) || !level_ok(a_level) || !level_ok(b_level) || !level_ok(out_level))
        return refuse_const(LR_ERR_ARG, "a count, the operation, the receiver, a degree or a level is out of range");
    LR_TRY(check_moduli(kCombine, moduli, n_moduli));
    if (!scale_ok(a_scale) || !scale_ok(b_scale) || !scale_ok(out_scale)) return refuse_const(LR_ERR_ARG, "a scale is not finite and positive");
    // the receiver that is an operand is that operand
    const bool out_is_a = receiver == LR_COMBINE_OUT_A || receiver == LR_COMBINE_OUT_BOTH;
    const bool out_is_b = receiver == LR_COMBINE_OUT_B || receiver == LR_COMBINE_OUT_BOTH;
    if ((out_is_a && (out_degree != a_degree || out_level != a_level || out_scale != a_scale)) ||
        (out_is_b && (out_degree != b_degree || out_level != b_level || out_scale != b_scale)))
        return refuse_const(LR_ERR_ARG, "the receiver is an operand and differs from it in degree, level or scale");
    // in every branch of :243-322 the operand of the smaller scale is multiplied by uint64(larger / smaller)
    const int side = a_scale < b_scale ? 1 : b_scale < a_scale ? 2 : 0;
    const double ratio = side == 1 ? b_scale / a_scale : side == 2 ? a_scale / b_scale : 1;
    if (!(ratio >= 0 && ratio < kTwo63)) return refuse_const(LR_ERR_ARG, "a scale ratio is not below 2^63");

    // getElemAndCheckBinary :117, :121
    const int max_degree = std::max(a_degree, b_degree);
    if (a_degree + b_degree == 0) return refuse_const(LR_ERR_UNSUPPORTED, "both operands have degree 0");
    if (out_degree < max_degree) return refuse_const(LR_ERR_UNSUPPORTED, "the receiver's degree is below the larger operand degree");
    // DropLevel(ctOut, ctOut.Level() - min(c0.Level(), c1.Level())) :238: a receiver at level 0 is left alone (:903, the error is ignored),
    // one above the operands comes down to them, one below both makes the difference wrap and the slice at :910 run out of range
    const int min_ab = std::min(a_level, b_level);
    if (out_level > 0 && out_level < min_ab) return refuse_const(LR_ERR_UNSUPPORTED, "the receiver lies above level 0 and below both operand levels");
    const int level = std::min(min_ab, out_level);                                                                   // :231
    // the multiplied operand that is not the receiver goes into the evaluator's pool ciphertext of degree 1 (:106; :247, :274, :300,
    // :310): MultByConst's `for u := range ct0.Value()` (:711-716) indexes its third component out of range
    const bool side_is_out = (side == 1 && out_is_a) || (side == 2 && out_is_b);
    if (side && !side_is_out && (side == 1 ? a_degree : b_degree) == 2)
        return refuse_const(LR_ERR_UNSUPPORTED, "the operand to be multiplied has degree 2 and is not the receiver");

    // nothing was written so far
    *level_after = level;
    *scale_after = std::max(a_scale, b_scale);                                                                       // :328
    *degree_after = max_degree;                                                                                      // Resize :237
    *mult_side = side;
    // MultByConst(ct, uint64(ratio), ...).  uint64(ratio) != 0 (:249 ...) always holds here: larger / smaller >= 1 for finite positive scales
    if (side)
        for (int i = 0; i <= level; ++i) mult[i] = integer_multiplier_word(ratio, limb_of(moduli[i]));
    return LR_OK;
    });
}

extern "C" int lr_ckks_power_basis_schedule(const uint64_t *moduli, int n_moduli, double default_scale, int chebyshev, int c1_level,
                                            double c1_scale, int n_targets, const uint32_t *targets, int capacity, int *n_products,
                                            lr_ckks_basis_product *products, uint64_t *mult, uint64_t *add) {
    return guarded([&]() -> int {
    const auto refuse_sched = [](const char *what) { return refuse(kSchedule, LR_ERR_ARG, what); };
    if (!moduli || !n_products || (n_targets > 0 && !targets) || (capacity > 0 && (!products || !mult || !add))) return refuse_sched("null argument");
    if (n_moduli < 1 || n_targets < 0 || capacity < 0 || c1_level < 0 || c1_level >= n_moduli) return refuse_sched("a count or a level is out of range");
    for (int t = 0; t < n_targets; ++t)
        if (targets[t] == 0 || targets[t] > 65535) return refuse_sched("a target is 0 or above 65535");
    LR_TRY(check_moduli(kSchedule, moduli, n_moduli));
    if (!scale_ok(default_scale) || !scale_ok(c1_scale)) return refuse_sched("a scale is not finite and positive");

    Recursion rec;
    for (int t = 0; t < n_targets; ++t) rec.want(targets[t]);
    const int count = (int)rec.order.size();
    if (count > capacity) {
        *n_products = count;      // the one word a refused call writes: the caller sizes its buffers by it and calls again
        return refuse_sched("more products than capacity");
    }

    std::vector<lr_ckks_basis_product> v((size_t)count);
    std::vector<u64> v_mult((size_t)count * n_moduli, 0), v_add((size_t)count * n_moduli, 0);
    struct State { int level, layer; double scale; };
    const auto state = [&](u32 x) { return x == 1 ? State{c1_level, 0, c1_scale} : State{v[rec.at[x]].level_after, v[rec.at[x]].layer, v[rec.at[x]].scale_after}; };
    for (int k = 0; k < count; ++k) {
        lr_ckks_basis_product &P = v[k];
        P.n = rec.order[k];
        P.a = (P.n + 1) >> 1;                                                // uint64(math.Ceil(float64(n) / 2)), :81 / :73
        P.b = P.n >> 1;
        P.c = chebyshev ? P.a - P.b : 0;                                     // :75
        const State A = state(P.a), B = state(P.b);
        P.mul_level = std::min(A.level, B.level);                            // MulRelinNew :1005
        P.layer = 1 + std::max(A.layer, B.layer);
        double scale = A.scale * B.scale;                                    // :1038
        if (!scale_ok(scale)) return refuse_sched("a scale is not finite and positive");
        // Rescale(C[n], ckksContext.scale, C[n]), :938-961: nothing at level 0 (the error return is ignored), else the loop
        int level = P.mul_level;
        P.n_rescales = 0;
        while (level != 0 && scale >= (default_scale * (double)moduli[level]) / 2) {
            scale /= (double)moduli[level];
            --level;
            ++P.n_rescales;
        }
        P.level_after = level;
        P.scale_after = scale;
        P.tail = !chebyshev ? 0 : P.c == 0 ? 2 : 1;
        P.mult_side = 0;
        if (P.tail == 1) {
            // Add(C[n], C[n], C[n]) :92 keeps level and scale; Sub(C[n], C[c], C[n]) :98 with C[c] = C[1]
            int level_after = 0, degree_after = 0, side = 0;
            double scale_after = 0;
            const int rc = lr_ckks_combine_constants(moduli, n_moduli, LR_SUB, 1, level, scale, 1, c1_level, c1_scale, 1, level, scale, LR_COMBINE_OUT_A,
                                                     &level_after, &scale_after, &degree_after, &side, &v_mult[(size_t)k * n_moduli]);
            if (rc != LR_OK) return refuse_sched("a scale ratio is not below 2^63");      // (every other argument is inside its domain)
            P.level_after = level_after;
            P.scale_after = scale_after;
            P.mult_side = side;
        } else if (P.tail == 2) {
            // AddConst(C[n], -1, C[n]) :96: scaleUpExact(-1, scale, q_i), real, so one word for both halves; the scale stays
            for (int i = 0; i <= level; ++i) {
                u64 hi;
                half_constants(-1, 0, scale, limb_of(moduli[i]), &v_add[(size_t)k * n_moduli + i], &hi);
            }
        }
    }
    // nothing was written so far
    *n_products = count;
    std::copy(v.begin(), v.end(), products);
    std::copy(v_mult.begin(), v_mult.end(), mult);
    std::copy(v_add.begin(), v_add.end(), add);
    return LR_OK;
    });
}
