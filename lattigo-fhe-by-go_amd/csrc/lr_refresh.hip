// lr_refresh.hip -- the kernels of the collective Refresh (lr_refresh.cpp): the reduction of the multi-word signed masks into RNS rows
// (SetCoefficientsBigint, dckks/public_refresh.go:66-68), the fused share pass of dckks GenShares (:78-92), Recode's exact centred lift
// from Q_levelStart to all of Q (:114-136), and for dbfv the products in front of the inverse transforms (dbfv/public_refresh.go:117-122,
// :141-142) and lift (:199-205) with the additions that follow it.  The element passes are streaming passes (lr_stream.hpp), batch on
// blockIdx.z.  The noise is expanded by launch_ckks_expand and launch_bfv_noise, Aggregate is launch_fold.
//
// Recode works on mixed-radix digits (Garner) instead of the reference's big.Int: v = d_0 + d_1 q_0 + ... + d_ls q_0 ... q_(ls-1) with
// d_k < q_k is the same integer as PolyToBigint's, digit strings compare as the integers do, and v mod q_i is a Horner chain of word-size
// modular steps.  No multi-word value lives in registers: the ls + 1 digits of a coefficient sit in LDS, one column per lane.
#include "lr_stream.hpp"

namespace lr {

namespace {

// (r 2^64 + w) mod q for r < q and any word w: one step of big.Int.Mod over the words from the top
__device__ __forceinline__ u64 word_step(u64 r, u64 w, u64 two64, const LimbParams &lp) {
    return cred(bred(r, two64, lp.q, lp.bred_hi, lp.bred_lo) + bred_add(w, lp.q, lp.bred_hi), lp.q);
}

}  // namespace

__global__ __launch_bounds__(256) void refresh_mask_kernel(RefreshMaskLaunch L) {
    const int limb = blockIdx.y;
    const long long b = blockIdx.z;
    const LimbParams lp = L.lp[limb];
    const u64 q = lp.q, two64 = L.two64.v[limb];
    const int n = L.n, W = L.words;
    const u64 *pm = L.mask + b * (long long)W * n;
    u64 *po = L.out + b * L.out_stride + (long long)limb * n;
    LR_FOR_PAIRS(j, n) {                                         // (coeff_grid: one coefficient per lane)
        const u64 top = ld_stream(pm + (long long)(W - 1) * n + j);
        u64 r = bred_add(top, q, lp.bred_hi);
        if (top >> 63) r = cred(r + (q - two64), q);            // the top word is signed: top - 2^64
        for (int w = W - 2; w >= 0; --w) r = word_step(r, ld_stream(pm + (long long)w * n + j), two64, lp);
        st_stream(po + j, r);
    }
}

hipError_t launch_refresh_mask(const RefreshMaskLaunch &L, int limbs, int batch, hipStream_t stream) {
    if (const LaunchVerdict v = launch_verdict(L, limbs, batch)) return verdict_error(v);
    return launch_kernel(refresh_mask_kernel, coeff_grid(L.n, (unsigned)limbs, (unsigned)batch), dim3(256), 0, stream, L);
}

// MulCoeffsMontgomeryAndAdd (:78, :81), Add (:85, :89) and Neg (:92) in the reference's order, each addition with its CRed; Neg is q - x:
// a zero becomes q, as the reference stores it
__global__ __launch_bounds__(256) void refresh_ckks_share_kernel(RefreshCkksShareLaunch L) {
    const int limb = blockIdx.y;
    const long long b = blockIdx.z;
    const LimbParams lp = L.lp[limb];
    const u64 q = lp.q;
    const long long row = (long long)limb * L.n;
    const bool dec = limb < L.dec_limbs;
    const ulonglong2 *pm = row_in(L.mask, b, L.r_stride, row), *p0 = row_in(L.e0, b, L.r_stride, row), *p1 = row_in(L.e1, b, L.r_stride, row);
    const ulonglong2 *ps = row_in(L.sk, b, L.sk_stride, row), *pc = row_in(L.c1, b, L.c1_stride, row), *pa = row_in(L.crs, b, L.crs_stride, row);
    ulonglong2 *pd = row_out(L.dec, b, L.dec_stride, row), *pr = row_out(L.rec, b, L.rec_stride, row);
    const int pairs = L.n >> 1;
    LR_FOR_PAIRS(e, pairs) {
        const ulonglong2 m = ld_stream(pm + e), a = ld_stream(pa + e), e1 = ld_stream(p1 + e), s = ld_shared(ps, L.sk_stride, e);
        if (dec) {
            const ulonglong2 c = ld_stream(pc + e), e0 = ld_stream(p0 + e);
            st_stream(pd + e, add2(muladd2(m, s, c, q, lp.qinv), e0, q));
        }
        st_stream(pr + e, neg2(add2(muladd2(m, s, a, q, lp.qinv), e1, q), q));
    }
}

hipError_t launch_refresh_ckks_share(const RefreshCkksShareLaunch &L, int limbs, int batch, hipStream_t stream) {
    if (const LaunchVerdict v = launch_verdict(L, limbs, batch)) return verdict_error(v);
    return launch_kernel(refresh_ckks_share_kernel, pair_grid(L.n, (unsigned)limbs, (unsigned)batch), dim3(256), 0, stream, L);
}

// One coefficient per lane, T lanes per workgroup, the digits in LDS at [k][lane].  Digit k costs k Horner steps modulo q_k, an output row
// ls + 1 steps modulo q_i: (ls + 1) (ls / 2 + limbs - row0) steps of one BRed each per coefficient.
template <int T>
__global__ __launch_bounds__(T) void refresh_recode_kernel(RefreshRecodeLaunch L) {
    extern __shared__ __align__(16) u64 refresh_digits[];
    const int j = blockIdx.x * T + threadIdx.x, n = L.n, ls = L.ls, nl = L.limbs;
    if (j >= n) return;                                          // (no barrier below: a lane reads only its own column)
    const long long b = blockIdx.y;
    const u64 *pi = L.in + b * L.in_stride + j;
    u64 *po = L.out + b * L.out_stride + j;
    u64 *d = refresh_digits + threadIdx.x;
    for (int k = 0; k <= ls; ++k) {
        const u64 q = ld_const(&L.lp[k].q), hi = ld_const(&L.lp[k].bred_hi), lo = ld_const(&L.lp[k].bred_lo);
        const u64 a = bred_add(ld_stream(pi + (long long)k * n), q, hi);
        u64 u = 0;                                               // (d_0 + d_1 q_0 + ... + d_(k-1) q_0 ... q_(k-2)) mod q_k
        for (int m = k - 1; m >= 0; --m) u = cred(bred(u, ld_const(L.qmod + k * nl + m), q, hi, lo) + bred_add(d[m * T], q, hi), q);
        d[k * T] = k ? bred(cred(a + (q - u), q), ld_const(L.ginv + k), q, hi, lo) : a;
    }
    // :130-133: Cmp(QHalf) is 1 or 0 => v -= Q_ls; the digit strings compare from the top as the integers do
    bool neg = true;
    for (int k = ls; k >= 0; --k) {
        const u64 x = d[k * T], h = ld_const(L.hdig + k);
        if (x != h) {
            neg = x > h;
            break;
        }
    }
    for (int i = L.row0; i < nl; ++i) {
        const u64 q = ld_const(&L.lp[i].q), hi = ld_const(&L.lp[i].bred_hi), lo = ld_const(&L.lp[i].bred_lo);
        u64 r = 0;
        for (int k = ls; k >= 0; --k) r = cred(bred(r, ld_const(L.qmod + i * nl + k), q, hi, lo) + bred_add(d[k * T], q, hi), q);
        if (neg) r = cred(r + (q - ld_const(L.qls + i)), q);
        st_stream(po + (long long)i * n, r);
    }
}

hipError_t launch_refresh_recode(const RefreshRecodeLaunch &L, int batch, hipStream_t stream) {
    if (const LaunchVerdict v = launch_verdict(L, batch)) return verdict_error(v);
    // 32 KiB of LDS at the most: 256 lanes up to 16 digits, 64 lanes beyond
    if (L.ls + 1 <= 16)
        return launch_kernel(refresh_recode_kernel<256>, dim3((unsigned)((L.n + 255) / 256), (unsigned)batch), dim3(256),
                             (size_t)(L.ls + 1) * 256 * sizeof(u64), stream, L);
    return launch_kernel(refresh_recode_kernel<64>, dim3((unsigned)((L.n + 63) / 64), (unsigned)batch), dim3(64),
                         (size_t)(L.ls + 1) * 64 * sizeof(u64), stream, L);
}

__global__ __launch_bounds__(256) void refresh_bfv_product_kernel(RefreshBfvProductLaunch L) {
    const int limb = blockIdx.y;
    const long long b = blockIdx.z;
    const LimbParams lp = L.lp[limb];
    const u64 q = lp.q;
    const long long row = (long long)limb * L.n;
    const bool inQ = limb < L.nQ;
    const u64 pm = inQ ? L.pmont.v[limb] : 0;
    const ulonglong2 *ps = row_in(L.sk, b, L.sk_stride, row);
    ulonglong2 *pa = row_out(L.a, b, L.stride, row), *pb = row_out(L.b, b, L.stride, row);
    const int pairs = L.n >> 1;
    LR_FOR_PAIRS(e, pairs) {
        const ulonglong2 s = ld_shared(ps, L.sk_stride, e);
        if (inQ) st_stream(pa + e, muls2(mul2(s, ld_stream(pa + e), q, lp.qinv), pm, q, lp.qinv));
        st_stream(pb + e, neg2(mul2(s, ld_stream(pb + e), q, lp.qinv), q));                // Neg: a zero becomes q, as in skEncryptor.encrypt
    }
}

hipError_t launch_refresh_bfv_product(const RefreshBfvProductLaunch &L, int rows, int batch, hipStream_t stream) {
    if (const LaunchVerdict v = launch_verdict(L, rows, batch)) return verdict_error(v);
    return launch_kernel(refresh_bfv_product_kernel, pair_grid(L.n, (unsigned)rows, (unsigned)batch), dim3(256), 0, stream, L);
}

// MODE 0: dec = CRed(dec + m), rec = CRed((rec + q) - m) (Add :156, Sub :159); MODE 1: dec = CRed(m + plus) (Add :185)
template <int MODE>
__global__ __launch_bounds__(256) void refresh_bfv_lift_kernel(RefreshBfvLiftLaunch L) {
    const int limb = blockIdx.y;
    const long long b = blockIdx.z;
    const LimbParams lp = L.lp[limb];
    const u64 q = lp.q, delta = L.delta_mont[limb];
    const long long row = (long long)limb * L.n;
    const ulonglong2 *pm = row_in(L.row, b, L.n, 0);
    ulonglong2 *pd = row_out(L.dec, b, L.dec_stride, row);
    ulonglong2 *pr = MODE == 0 ? row_out(L.rec, b, L.rec_stride, row) : nullptr;
    const ulonglong2 *pp = MODE == 1 ? row_in(L.plus, b, L.plus_stride, row) : nullptr;
    const int pairs = L.n >> 1;
    LR_FOR_PAIRS(e, pairs) {
        const ulonglong2 m = muls2(pm[e], delta, q, lp.qinv);    // (the row is read once per limb: through the caches)
        if constexpr (MODE == 0) {
            const ulonglong2 d = ld_stream(pd + e), r = ld_stream(pr + e);
            st_stream(pd + e, add2(d, m, q));
            st_stream(pr + e, sub2(r, m, q));
        } else {
            st_stream(pd + e, add2(m, ld_stream(pp + e), q));
        }
    }
}

hipError_t launch_refresh_bfv_lift(const RefreshBfvLiftLaunch &L, int limbs, int batch, hipStream_t stream) {
    if (const LaunchVerdict v = launch_verdict(L, limbs, batch)) return verdict_error(v);
    const dim3 grid = pair_grid(L.n, (unsigned)limbs, (unsigned)batch);
    return L.rec ? launch_kernel(refresh_bfv_lift_kernel<0>, grid, dim3(256), 0, stream, L) : launch_kernel(refresh_bfv_lift_kernel<1>, grid, dim3(256), 0, stream, L);
}

}  // namespace lr
