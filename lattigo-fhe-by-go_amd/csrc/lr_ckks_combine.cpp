// lr_ckks_combine.cpp -- C ABI: out = a (+|-) b for CKKS ciphertexts of any scale, level and degree, evaluator.Add / AddNoMod / Sub /
// SubNoMod through evaluateInPlace (ckks/evaluator.go:153-342), and the steps of the same shape between the products of polynomial and
// Chebyshev evaluation.
//   lr_ckks_combine_constants   the scalar side, host only (no context, no device): which operand is multiplied and by which words, the
//                               level, scale and degree of the result, what the reference panics on
//   lr_ckks_combine             the element side, one streaming pass (lr_ckks_combine.hip)
// The unit's name keeps it out of the lr_abi_*.cpp set that the shared sanitizer build links against its fixed launch stubs: the launcher
// it calls has a stand-in of its own (tests/cpp/ckks_combine_stub.cpp).
#include "lr_ckks_scalar.hpp"

namespace lr_host {
namespace {
using namespace ckks_scalar;

const char *const kWho = "CKKS combine: ";
const char *const kWhoConst = "CKKS combine constants: ";

int refuse_const(int code, const char *what) { return fail(code, std::string(kWhoConst) + what); }
int refuse(int code, const char *what) { return fail(code, std::string(kWho) + what); }

// the very poly: the in-place case of the reference (the same component of the same ciphertext)
bool same_poly(const lr_poly *p, const lr_poly *o) { return p == o || (p->d == o->d && p->batch == o->batch && p->stride() == o->stride()); }

}  // namespace
}  // namespace lr_host

extern "C" int lr_ckks_combine_constants(const uint64_t *moduli, int n_moduli, int op, int a_degree, int a_level, double a_scale, int b_degree,
                                         int b_level, double b_scale, int out_degree, int out_level, double out_scale, int receiver,
                                         int *level_after, double *scale_after, int *degree_after, int *mult_side, uint64_t *mult) {
    return guarded([&]() -> int {
    if (!moduli || !level_after || !scale_after || !degree_after || !mult_side || !mult) return refuse_const(LR_ERR_ARG, "null argument");
    const auto degree_ok = [](int d) { return d >= 0 && d <= 2; };
    const auto level_ok = [&](int l) { return l >= 0 && l < n_moduli; };
    if (n_moduli < 1 || op < LR_ADD || op > LR_SUB_NOMOD || receiver < LR_COMBINE_OUT_NEW || receiver > LR_COMBINE_OUT_BOTH || !degree_ok(a_degree) ||
        !degree_ok(b_degree) || !degree_ok(out_degree) || !level_ok(a_level) || !level_ok(b_level) || !level_ok(out_level))
        return refuse_const(LR_ERR_ARG, "a count, the operation, the receiver, a degree or a level is out of range");
    for (int i = 0; i < n_moduli; ++i)
        if (moduli[i] < 3 || !(moduli[i] & 1) || (moduli[i] >> 61)) return refuse_const(LR_ERR_ARG, "a modulus is even, below 3 or not below 2^61");
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
    if (side) {
        // MultByConst(ct, uint64(ratio), ...): the uint64 becomes a float64 again (:669-671), scale 1, no imaginary part (:698-709).
        // uint64(ratio) != 0 (:249 ...) always holds here: larger / smaller >= 1 for finite positive scales
        const double c_real = (double)(u64)ratio;
        for (int i = 0; i <= level; ++i) {
            const Limb m{moduli[i], montgomery_const(moduli[i]), 0, barrett_const(moduli[i])};
            u64 unused;
            half_constants_mform(c_real, 0, 1, m, &mult[i], &unused);
        }
    }
    return LR_OK;
    });
}

extern "C" int lr_ckks_combine(lr_context *c, int op, int level, int a_degree, const lr_poly *const *a, int b_degree, const lr_poly *const *b,
                               int double_a, const uint64_t *ma_lo, const uint64_t *ma_hi, const uint64_t *mb_lo, const uint64_t *mb_hi,
                               const uint64_t *add_lo, const uint64_t *add_hi, lr_poly *const *out) {
    return guarded([&]() -> int {
    // LR_ERR_ARG
    if (!c || !out) return refuse(LR_ERR_ARG, "null argument");
    if (!a) return refuse(LR_ERR_ARG, "no operand given");
    if (op < LR_ADD || op > LR_SUB_NOMOD) return refuse(LR_ERR_ARG, "the operation is not LR_ADD, LR_ADD_NOMOD, LR_SUB or LR_SUB_NOMOD");
    if (a_degree < 0 || a_degree > 2 || (b && (b_degree < 0 || b_degree > 2))) return refuse(LR_ERR_ARG, "a degree is outside 0..2");
    const int deg_b = b ? b_degree : -1, comps = combine_comps(a_degree, deg_b);
    for (int u = 0; u <= a_degree; ++u)
        if (!a[u]) return refuse(LR_ERR_ARG, "a component is null");
    for (int u = 0; u <= deg_b; ++u)
        if (!b[u]) return refuse(LR_ERR_ARG, "a component is null");
    for (int u = 0; u < comps; ++u)
        if (!out[u]) return refuse(LR_ERR_ARG, "a component is null");
    if ((ma_lo == nullptr) != (ma_hi == nullptr) || (mb_lo == nullptr) != (mb_hi == nullptr) || (add_lo == nullptr) != (add_hi == nullptr))
        return refuse(LR_ERR_ARG, "the two words of a multiplier or of the constant come together or not at all");
    if (!b && mb_lo) return refuse(LR_ERR_ARG, "a multiplier of b without b");
    // out_u may be the very poly a_u or b_u; nothing else of the receiver may share memory with anything
    for (int u = 0; u < comps; ++u)
        for (int v = u + 1; v < comps; ++v)
            if (out[u] == out[v] || overlap(out[u], out[v])) return refuse(LR_ERR_ARG, "the components of the receiver share memory");
    for (int u = 0; u < comps; ++u) {
        for (int v = 0; v <= a_degree; ++v)
            if (overlap(a[v], out[u]) && !(u == v && same_poly(a[v], out[u])))
                return refuse(LR_ERR_ARG, "an operand shares memory with the receiver other than component by component in place");
        for (int v = 0; v <= deg_b; ++v)
            if (overlap(b[v], out[u]) && !(u == v && same_poly(b[v], out[u])))
                return refuse(LR_ERR_ARG, "an operand shares memory with the receiver other than component by component in place");
    }
    // LR_ERR_SHAPE
    if (level < 0 || level + 1 > c->h.L()) return refuse(LR_ERR_SHAPE, "level out of range");
    const int batch = out[0]->batch;
    const auto shape = [&](const lr_poly *p, bool operand) -> int {
        if (p->N != c->h.N) return refuse(LR_ERR_SHAPE, "ring degree mismatch");
        if (level + 1 > p->limbs) return refuse(LR_ERR_SHAPE, "a poly has fewer limbs than level + 1");
        if (p->batch != batch && !(operand && p->batch == 1))
            return refuse(LR_ERR_SHAPE, "the receiver's components carry one batch, an operand that batch or 1");
        return LR_OK;
    };
    for (int u = 0; u < comps; ++u) LR_TRY(shape(out[u], false));
    for (int u = 0; u <= a_degree; ++u) LR_TRY(shape(a[u], true));
    for (int u = 0; u <= deg_b; ++u) LR_TRY(shape(b[u], true));
    if (batch > 32767) return refuse(LR_ERR_SHAPE, "batch above 32767");
    if ((long long)comps * batch > 65535) return refuse(LR_ERR_SHAPE, "batch above 21845 at degree 2");
    // LR_ERR_UNSUPPORTED
    if (c->h.N < 4) return refuse(LR_ERR_UNSUPPORTED, "ring degree below 4");

    LR_HIP(hipSetDevice(c->device));
    CombineLaunch L;
    std::memset(&L, 0, sizeof L);
    const auto stride = [&](const lr_poly *p) { return p->batch == 1 && batch > 1 ? 0ll : p->stride(); };       // one poly read by every member
    for (int u = 0; u <= a_degree; ++u) {
        L.a[u] = a[u]->d;
        L.a_stride[u] = stride(a[u]);
    }
    for (int u = 0; u <= deg_b; ++u) {
        L.b[u] = b[u]->d;
        L.b_stride[u] = stride(b[u]);
    }
    for (int u = 0; u < comps; ++u) {
        L.out[u] = out[u]->d;
        L.out_stride[u] = out[u]->stride();
    }
    L.n = (int)c->h.N;
    L.op = op;
    L.deg_a = a_degree;
    L.deg_b = deg_b;
    L.double_a = double_a ? 1 : 0;
    L.mult_a = ma_lo ? 1 : 0;
    L.mult_b = mb_lo ? 1 : 0;
    L.has_add = add_lo ? 1 : 0;
    L.lp = c->d_lp;
    for (int i = 0; i <= level; ++i) {
        u64 *w = L.k + (size_t)i * kCombineLimbWords;
        if (ma_lo) w[0] = ma_lo[i], w[1] = ma_hi[i];
        if (mb_lo) w[2] = mb_lo[i], w[3] = mb_hi[i];
        if (add_lo) w[4] = add_lo[i], w[5] = add_hi[i];
    }
    LR_HIP(launch_ckks_combine(L, level + 1, batch, c->stream));
    return LR_OK;
    });
}
