// lr_stream.hpp -- the streaming pass that the element-wise kernel families share (lr_ewise.hip, the two encryptors, the key generator,
// collective key switching, Refresh, collective setup); included by .hip files only.
//
// A streaming pass is HBM-bound: every poly element is read or written once.  16 B per lane per access to poly data, two coefficients per
// lane (one ulonglong2), the limb on blockIdx.y so that the per-modulus constants are wave-uniform (SGPRs), the batch member -- a poly, a
// key, a party x digit -- on blockIdx.z, and a grid-stride loop over the coefficient pairs of one row.  Its rules, each stated here once:
//   1. the grid of a pass and the loop that walks it (pair_grid / LR_FOR_PAIRS; coeff_grid for one coefficient per lane);
//   2. an operand's row as a 16-byte pointer (row_in / row_out), and whether its load streams past the caches (ld_shared);
//   3. pair arithmetic with the reference's CRed placement (add2 ... times_p2);
//   4. ring.PermuteNTTIndex for one position (galois_index);
//   5. the samplers' wire formats: ternary bit planes (ternary_pair) and the Gaussian sign-magnitude byte (noise_residue / noise_operand).
// A new handle's kernels start from these; a kernel keeps what is its own: its operands, its formula, its reference lines.
#pragma once
#include "lr_device.hpp"

namespace lr {

// ---- 1. grid and loop ----
// workgroups of 256 lanes over the pairs of one row: enough to cover the row up to 64, beyond that the lanes make further trips (at
// N = 2^16: two), and never an empty grid
inline int pair_blocks(int n) {
    int gx = ((n >> 1) + 255) / 256;
    if (gx > 64) gx = 64;
    if (gx < 1) gx = 1;
    return gx;
}
inline dim3 pair_grid(int n, unsigned y, unsigned z) { return dim3((unsigned)pair_blocks(n), y, z); }
// the same with one coefficient per lane (kernels that gather or scatter single words)
inline dim3 coeff_grid(int n, unsigned y, unsigned z) { return pair_grid(2 * n, y, z); }
// the loop of a lane over its share of `count` pairs (coeff_grid: coefficients); the trip stride is the grid's width in lanes
#define LR_FOR_PAIRS(e, count) for (int e = blockIdx.x * 256 + threadIdx.x; e < (count); e += gridDim.x * 256)

// ---- 2. operands ----
// row `row` (in words: limb * n) of member b of an operand whose members lie `stride` words apart
LR_D const ulonglong2 *row_in(const u64 *base, long long b, long long stride, long long row) {
    return reinterpret_cast<const ulonglong2 *>(base + b * stride + row);
}
LR_D ulonglong2 *row_out(u64 *base, long long b, long long stride, long long row) { return reinterpret_cast<ulonglong2 *>(base + b * stride + row); }
// An operand that the whole batch shares (stride 0: a key, a common reference poly) is read by every member: through the caches.  One that
// each member owns is read once: it streams past them (ld_stream) and leaves the tables and keys in L2 and the Infinity Cache alone.
LR_D ulonglong2 ld_shared(const ulonglong2 *p, long long stride, int e) { return stride ? ld_stream(p + e) : p[e]; }

// ---- 3. pair arithmetic: the element operations of ring/ring.go on both coefficients of a lane ----
// (each keeps the reference's reduction: CRed where Context.Add / Sub have it, none where Neg has none)
LR_D ulonglong2 add2(ulonglong2 a, ulonglong2 b, u64 q) { return make_ulonglong2(cred(a.x + b.x, q), cred(a.y + b.y, q)); }
// Context.Sub: CRed((a + q) - b); equal operands give CRed(q) = 0
LR_D ulonglong2 sub2(ulonglong2 a, ulonglong2 b, u64 q) { return make_ulonglong2(cred((a.x + q) - b.x, q), cred((a.y + q) - b.y, q)); }
// Context.AddNoMod / SubNoMod (ring/ring.go:48, :94): the same sums left unreduced
LR_D ulonglong2 add2_nomod(ulonglong2 a, ulonglong2 b) { return make_ulonglong2(a.x + b.x, a.y + b.y); }
LR_D ulonglong2 sub2_nomod(ulonglong2 a, ulonglong2 b, u64 q) { return make_ulonglong2((a.x + q) - b.x, (a.y + q) - b.y); }
// Context.Neg: q - x without reduction, so a zero becomes q, as the reference stores it
LR_D ulonglong2 neg2(ulonglong2 a, u64 q) { return make_ulonglong2(q - a.x, q - a.y); }
LR_D ulonglong2 mul2(ulonglong2 a, ulonglong2 b, u64 q, u64 qinv) { return make_ulonglong2(mred(a.x, b.x, q, qinv), mred(a.y, b.y, q, qinv)); }
// MulScalar: MRed by one Montgomery-form scalar
LR_D ulonglong2 muls2(ulonglong2 a, u64 s, u64 q, u64 qinv) { return make_ulonglong2(mred(a.x, s, q, qinv), mred(a.y, s, q, qinv)); }
// CRed(x + MRed(a, b)): MulCoeffsMontgomeryAndAdd (ring/ring.go:283)
LR_D ulonglong2 muladd2(ulonglong2 x, ulonglong2 a, ulonglong2 b, u64 q, u64 qinv) {
    return make_ulonglong2(cred(x.x + mred(a.x, b.x, q, qinv), q), cred(x.y + mred(a.y, b.y, q, qinv), q));
}
// CRed(x + (q - MRed(a, b))): MulCoeffsMontgomeryAndSub (ring/ring.go:311)
LR_D ulonglong2 mulsub2(ulonglong2 x, ulonglong2 a, ulonglong2 b, u64 q, u64 qinv) {
    return make_ulonglong2(cred(x.x + (q - mred(a.x, b.x, q, qinv)), q), cred(x.y + (q - mred(a.y, b.y, q, qinv)), q));
}
LR_D ulonglong2 mform2(ulonglong2 a, const LimbParams &lp) {
    return make_ulonglong2(mform(a.x, lp.q, lp.bred_hi, lp.bred_lo), mform(a.y, lp.q, lp.bred_hi, lp.bred_lo));
}
// InvMForm(MulScalarBigint(s, P)) (dbfv/relinkey_gen.go:225-227): MRed by MForm(P mod q), then out of Montgomery form
LR_D u64 times_p(u64 s, u64 pm, u64 q, u64 qinv) { return inv_mform(mred(s, pm, q, qinv), q, qinv); }
LR_D ulonglong2 times_p2(u64 s0, u64 s1, u64 pm, u64 q, u64 qinv) { return make_ulonglong2(times_p(s0, pm, q, qinv), times_p(s1, pm, q, qinv)); }

// ---- 4. ring.PermuteNTTIndex (ring/ring_galois.go:29-52) for one position: PermuteNTT is out[j] = in[galois_index(j)] ----
// gen odd, reduced modulo 2 N; mask2 = 2 N - 1 (two bit reversals, no table)
LR_D u32 galois_index(u32 j, u32 gen, u32 mask2, int logn) {
    const u32 t1 = 2 * (__brev(j) >> (32 - logn)) + 1;
    const u32 t2 = (((gen * t1) & mask2) - 1) >> 1;
    return __brev(t2) >> (32 - logn);
}

// ---- 5. the samplers' compact decisions ----
// sampleTernary's two bit planes (TernaryLaunch): coefficient i takes bit i & 7 of byte i >> 3 of each plane.  Pair e holds coefficients 2e
// and 2e + 1: both bits of a plane sit in byte e >> 2 at bit 2 (e & 3), so a lane takes its two decisions from one byte load per plane
// (four neighbouring lanes share the byte) and a wave's 16-byte stores stay contiguous.
// index 0 -> 0, 1 (coeff, sign 0) -> MForm(1), 2 (coeff, sign 1) -> MForm(q - 1)
LR_D u64 ternary_value(unsigned c, unsigned s, u64 one, u64 minus_one) { return (c & 1) ? ((s & 1) ? minus_one : one) : 0; }
LR_D ulonglong2 ternary_pair(const unsigned char *coeff_plane, const unsigned char *sign_plane, int e, u64 one, u64 minus_one) {
    const unsigned sh = (unsigned)(e & 3) * 2;
    const unsigned c = (unsigned)coeff_plane[e >> 2] >> sh, s = (unsigned)sign_plane[e >> 2] >> sh;
    return make_ulonglong2(ternary_value(c, s, one, minus_one), ternary_value(c >> 1, s >> 1, one, minus_one));
}
// The Gaussian samplers' byte: low 7 bits the magnitude c, bit 7 the sign; the residue is sign 1 -> c, sign 0 -> q - c
// (ring/gaussianSampler.go:247,271).  The two decodes differ in one value, (0, sign 0): noise_residue keeps the reference's q, because its
// result is stored or added as it is; noise_operand writes 0, because a forward transform takes it next and Context.NTT ends on a full
// reduction, so no bit of the transform's result changes.
LR_D u64 noise_residue(unsigned byte, u64 q) {
    const u64 c = byte & 127u;
    return (byte & 128u) ? c : q - c;
}
LR_D u64 noise_operand(unsigned byte, u64 q) {
    const u64 c = byte & 127u;
    return (byte & 128u) || c == 0 ? c : q - c;
}

}  // namespace lr
