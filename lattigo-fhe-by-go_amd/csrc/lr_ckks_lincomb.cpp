// lr_ckks_lincomb.cpp -- C ABI: res = c0 + sum_k c_k ct_k for CKKS ciphertexts of degree 1, the leaf of the reference's polynomial
// evaluation (evaluatePolyFromPowerBasis, ckks/polynomial_evaluation.go:142-159: one AddConst and a chain of MultByConstAndAdd).
//   lr_ckks_lincomb_constants   the scalar side of that chain, host only (no context, no device): levels, scales and the per-limb words
//   lr_ckks_lincomb             the element side, one streaming pass per sixteen terms (lr_ckks_lincomb.hip)
// The unit's name keeps it out of the lr_abi_*.cpp set that the shared sanitizer build links against its fixed launch stubs: the launcher
// it calls has a stand-in of its own (tests/cpp/ckks_lincomb_stub.cpp).
#include "lr_ckks_scalar.hpp"

namespace lr_host {
namespace {
using namespace ckks_scalar;      // the scalar side: scaleUpExact, the half-vector words, the domain (shared with lr_ckks_combine.cpp)

const char *const kWho = "CKKS linear combination: ";
const char *const kWhoConst = "CKKS linear combination constants: ";

int refuse_const(const char *what) { return fail(LR_ERR_ARG, std::string(kWhoConst) + what); }

int refuse(int code, const char *what) { return fail(code, std::string(kWho) + what); }

}  // namespace
}  // namespace lr_host

extern "C" int lr_ckks_lincomb_constants(const uint64_t *moduli, const uint64_t *ntt_psi1, int n_moduli, double default_scale, int res_level,
                                         double res_scale, int has_const, double c0_re, double c0_im, int n_terms, const double *term_re,
                                         const double *term_im, const double *term_scale, const int *term_level, int *level_after,
                                         double *scale_after, uint64_t *add_lo, uint64_t *add_hi, uint8_t *has_pre, uint64_t *pre, uint64_t *lo,
                                         uint64_t *hi) {
    return guarded([&]() -> int {
    if (!moduli || !ntt_psi1 || !level_after || !scale_after) return refuse_const("null argument");
    if (has_const && (!add_lo || !add_hi)) return refuse_const("null argument");
    if (n_terms > 0 && (!term_re || !term_im || !term_scale || !term_level || !has_pre || !pre || !lo || !hi)) return refuse_const("null argument");
    if (n_moduli < 1 || n_terms < 0 || res_level < 0 || res_level >= n_moduli) return refuse_const("a count or a level is out of range");
    for (int k = 0; k < n_terms; ++k)
        if (term_level[k] < 0 || term_level[k] >= n_moduli) return refuse_const("a count or a level is out of range");
    for (int i = 0; i < n_moduli; ++i) {
        if (moduli[i] < 3 || !(moduli[i] & 1) || (moduli[i] >> 61)) return refuse_const("a modulus is even, below 3 or not below 2^61");
        if (ntt_psi1[i] >= moduli[i]) return refuse_const("a root word is not below its modulus");
    }
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
    for (int i = 0; i < L1; ++i) limb[i] = Limb{moduli[i], montgomery_const(moduli[i]), ntt_psi1[i], barrett_const(moduli[i])};
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
                    const double c_real = (double)(u64)ratio;
                    v_has_pre[k] = 1;
                    for (int i = 0; i < L1; ++i) {
                        u64 unused;
                        half_constants_mform(c_real, 0, 1, limb[i], &pre_k[i], &unused);
                    }
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

extern "C" int lr_ckks_lincomb(lr_context *c, int level, int n_terms, const lr_poly *const *terms_c0, const lr_poly *const *terms_c1,
                               const uint8_t *has_pre, const uint64_t *pre, const uint64_t *lo, const uint64_t *hi, const uint64_t *add_lo,
                               const uint64_t *add_hi, int accumulate, lr_poly *out_c0, lr_poly *out_c1) {
    return guarded([&]() -> int {
    // LR_ERR_ARG
    if (!c || !out_c0 || !out_c1) return refuse(LR_ERR_ARG, "null argument");
    if (n_terms < 0) return refuse(LR_ERR_ARG, "n_terms is negative");
    if (n_terms > 0 && (!terms_c0 || !terms_c1 || !has_pre || !pre || !lo || !hi)) return refuse(LR_ERR_ARG, "null argument");
    for (int k = 0; k < n_terms; ++k)
        if (!terms_c0[k] || !terms_c1[k]) return refuse(LR_ERR_ARG, "a term is null");
    if ((add_lo == nullptr) != (add_hi == nullptr)) return refuse(LR_ERR_ARG, "add_lo and add_hi come together or not at all");
    if (out_c0 == out_c1 || overlap(out_c0, out_c1)) return refuse(LR_ERR_ARG, "the two components of the receiver share memory");
    for (int k = 0; k < n_terms; ++k)
        for (const lr_poly *t : {terms_c0[k], terms_c1[k]})
            if (overlap(t, out_c0) || overlap(t, out_c1)) return refuse(LR_ERR_ARG, "a term shares memory with the receiver");
    // LR_ERR_SHAPE
    const int batch = out_c0->batch;
    const auto shape = [&](const lr_poly *p) -> int {
        if (p->N != c->h.N) return refuse(LR_ERR_SHAPE, "ring degree mismatch");
        if (level + 1 > p->limbs) return refuse(LR_ERR_SHAPE, "a poly has fewer limbs than level + 1");
        if (p->batch != batch) return refuse(LR_ERR_SHAPE, "every term and the receiver carry the same batch");
        return LR_OK;
    };
    if (level < 0 || level + 1 > c->h.L()) return refuse(LR_ERR_SHAPE, "level out of range");
    LR_TRY(shape(out_c0));
    LR_TRY(shape(out_c1));
    for (int k = 0; k < n_terms; ++k) {
        LR_TRY(shape(terms_c0[k]));
        LR_TRY(shape(terms_c1[k]));
    }
    if (batch > 32767) return refuse(LR_ERR_SHAPE, "batch above 32767");
    // LR_ERR_UNSUPPORTED
    if (c->h.N < 4) return refuse(LR_ERR_UNSUPPORTED, "ring degree below 4");

    if (n_terms == 0 && !add_lo && accumulate) return LR_OK;      // the receiver as it is
    LR_HIP(hipSetDevice(c->device));
    const int L1 = level + 1;
    // kLinCombTerms terms per pass, the constant on the first, every further pass on top of the receiver; within a pass as many limbs per
    // launch as its constants leave room for in the kernel arguments
    int first = 0;
    do {
        const int count = std::min(n_terms - first, kLinCombTerms);
        LinCombLaunch L;
        std::memset(&L, 0, sizeof L);
        for (int k = 0; k < count; ++k) {
            const lr_poly *t0 = terms_c0[first + k], *t1 = terms_c1[first + k];
            L.term[k] = LinCombTermRef{{t0->d, t1->d}, {t0->stride(), t1->stride()}};
            if (has_pre[first + k]) L.pre_mask |= 1u << k;
        }
        L.out[0] = out_c0->d;
        L.out[1] = out_c1->d;
        L.out_stride[0] = out_c0->stride();
        L.out_stride[1] = out_c1->stride();
        L.n = (int)c->h.N;
        L.count = count;
        L.accumulate = first > 0 || accumulate ? 1 : 0;
        L.has_add = first == 0 && add_lo ? 1 : 0;
        L.lp = c->d_lp;
        const int words = lincomb_limb_words(count, L.has_add), step = lincomb_limbs_per_launch(count, L.has_add);
        for (int limb0 = 0; limb0 < L1; limb0 += step) {
            const int limbs = std::min(step, L1 - limb0);
            L.limb0 = limb0;
            for (int y = 0; y < limbs; ++y) {
                u64 *w = L.k + (size_t)y * words;
                const int i = limb0 + y;
                if (L.has_add) {
                    *w++ = add_lo[i];
                    *w++ = add_hi[i];
                }
                for (int k = 0; k < count; ++k) {
                    const size_t at = (size_t)(first + k) * L1 + i;
                    *w++ = L.pre_mask >> k & 1u ? pre[at] : 0;
                    *w++ = lo[at];
                    *w++ = hi[at];
                }
            }
            LR_HIP(launch_ckks_lincomb(L, limbs, batch, c->stream));
        }
        first += count;
    } while (first < n_terms);
    return LR_OK;
    });
}
