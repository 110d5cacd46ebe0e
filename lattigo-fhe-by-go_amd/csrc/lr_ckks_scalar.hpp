// lr_ckks_scalar.hpp -- the scalar lines that ckks.Evaluator's constant-by-ciphertext methods share (AddConst, MultByConst,
// MultByConstAndAdd; ckks/evaluator.go:373-734), restated for one modulus on the host: scaleUpExact, the two half-vector words before and
// after MForm, and the domain on which Go's float-to-integer conversions are defined.  Included by the host-only constants functions
// (lr_abi_ckks_scalar.cpp); no context, no device, no state.
#pragma once
#include <cmath>

#include "lr_host.hpp"

namespace lr_host {
namespace ckks_scalar {

const double kTwo63 = 9223372036854775808.0;

// Go's uint64(f) / int64(f) are machine-specific out of range: the domain ends below 2^63 on either side
inline bool magnitude_ok(double f) { return std::isfinite(f) && std::fabs(f) < kTwo63; }
inline bool scale_ok(double f) { return std::isfinite(f) && f > 0; }

// the integer part of a finite w >= 0, modulo q: below 2^64 the truncated word, above it mant * 2^e with e >= 12
inline u64 trunc_mod(double w, u64 q) {
    if (w < 18446744073709551616.0) return (u64)w % q;
    int e2 = 0;
    const double m = std::frexp(w, &e2);                      // w = m * 2^e2, 0.5 <= m < 1
    const u64 mant = (u64)std::ldexp(m, 53);                  // exact: 53 bits
    u128 p = 1 % q, b = 2 % q;
    for (int e = e2 - 53; e; e >>= 1) {
        if (e & 1) p = p * b % q;
        b = b * b % q;
    }
    return (u64)((u128)(mant % q) * p % q);
}

// scaleUpExact (ckks/utils.go:22-49): big.NewFloat has 53 bits, so n * value and the + 0.5 round as doubles do (ties to even), Int()
// truncates, and a negative value whose remainder is zero gives q, not 0.  The restatement the CKKS encoder's kernel carries
// (scale_up_store, lr_ckks_encode.hip), for one modulus on the host.
inline u64 scale_up_exact(double value, double n, u64 q) {
    const bool neg = value < 0;
    const double y = neg ? -n * value : n * value;
    const u64 r = trunc_mod(y + 0.5, q);
    return neg ? q - r : r;
}

// "determines if a scaling is required (which is the case if either real or imag have a rational part)", :466-488, :632-654
inline bool has_fraction(double v) {
    if (v == 0) return false;
    const int64_t value_int = (int64_t)v;
    return v - (double)value_int != 0;
}

struct Limb {
    u64 q, qinv, psi;
    BarrettConst bred;
};
// psi = the limb's root word (ntt_psi1); 0 where every constant is real
inline Limb limb_of(u64 q, u64 psi = 0) { return Limb{q, montgomery_const(q), psi, barrett_const(q)}; }

// scaledConst for the coefficients below and above N / 2, before any MForm (:413-427, :436-438; :570-583, :595-596; :694-707, :719-720)
inline void half_constants(double re, double im, double scale, const Limb &m, u64 *lo, u64 *hi) {
    u64 sc = 0, sc_real = 0, sc_imag = 0;
    if (re != 0) {
        sc_real = scale_up_exact(re, scale, m.q);
        sc = sc_real;
    }
    if (im != 0) {
        sc_imag = mred(scale_up_exact(im, scale, m.q), m.psi, m.q, m.qinv);
        sc = cred(sc + sc_imag, m.q);
    }
    *lo = sc;
    if (im != 0) sc = cred(sc_real + (m.q - sc_imag), m.q);
    *hi = sc;
}

// the same after MForm (:585, :597; :709, :721): with a real constant the second half keeps the first half's word
inline void half_constants_mform(double re, double im, double scale, const Limb &m, u64 *lo, u64 *hi) {
    u64 l, h;
    half_constants(re, im, scale, m, &l, &h);
    *lo = mform(l, m.q, m.bred.hi, m.bred.lo);
    *hi = im != 0 ? mform(h, m.q, m.bred.hi, m.bred.lo) : *lo;
}

// MultByConst(ct, uint64(ratio), ...): the uint64 becomes a float64 again (:669-671), an integer constant at scale 1 with no imaginary
// part (:698-709), so one word serves both halves
inline u64 integer_multiplier_word(double ratio, const Limb &m) {
    u64 w, unused;
    half_constants_mform((double)(u64)ratio, 0, 1, m, &w, &unused);
    return w;
}

}  // namespace ckks_scalar
}  // namespace lr_host
