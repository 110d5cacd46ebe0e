// lr_ckks_encode.hip -- ckks.Encoder on the device (ckks/encoder.go:78-226, ckks/utils.go:51-114): a batch of plaintexts per launch.
//
// Both special FFTs have a fixed butterfly data flow, and every butterfly here does the reference's operations on IEEE doubles: a sum, a
// difference and the product (ac - bd, ad + bc) with the caller's root table, no multiply-add fused (the library is compiled with
// -ffp-contract=off).  Any schedule of the butterflies therefore gives the reference's bits, and the two routes only split the work:
//
// Fused route (slots <= 2^13): one workgroup per plaintext, the slots in LDS as a plane of real and a plane of imaginary parts
// (16 * slots bytes, 128 KiB of the CU's 160 at 2^13).  With split planes every access is an 8-byte one: at spans of 32 and more the 32 lanes
// of a group cover the 64 banks exactly once.  Smaller spans and the bit-reversed read-out collide (as interleaved elements would): accepted.
// Tiled route (larger slots, or Options::ckks_encoder_tiled): the stages whose span exceeds the tile stream over global memory, one stage
// per launch; the others run in LDS, one tile per workgroup.  The twiddle of a butterfly depends on its stage and its offset inside the
// stage's block alone, so a tile runs the very stage loop of the fused kernels.
//
// The integer ends: scale-up is scaleUpVecExact per coefficient and limb; ckks_crt_to_double is PolyToBigint + Mod + centring + scaleDown
// for one coefficient per thread on little-endian 64-bit words.
#include "lr_device.hpp"

#include <atomic>

namespace lr {

namespace {

constexpr int kCkksThreads = 1024;

__device__ __forceinline__ unsigned bit_reverse_of(unsigned i, int bits) { return bits ? __brev(i) >> (32 - bits) : 0u; }

__device__ __forceinline__ Cplx root_at(const CkksEncTables &tab, unsigned idx) {
    const double *p = (const double *)tab.roots + 2 * (size_t)idx;
    return Cplx{p[0], p[1]};
}

// the twiddle indices of encoder.go:181 and :217 for the stage len = 2^ll and the offset j in its block; lenq = 4 len divides m = 2 N
__device__ __forceinline__ unsigned dif_root_index(const CkksEncTables &tab, int ll, int j) {
    const unsigned lenq = 4u << ll, gap = (2u * (unsigned)tab.n) >> (ll + 2);
    return (lenq - (tab.rot[j] & (lenq - 1))) * gap;
}
__device__ __forceinline__ unsigned dit_root_index(const CkksEncTables &tab, int ll, int j) {
    const unsigned lenq = 4u << ll, gap = (2u * (unsigned)tab.n) >> (ll + 2);
    return (tab.rot[j] & (lenq - 1)) * gap;
}

// invfftlazy's butterfly (:182-186): u = a + b, v = (a - b) * w
__device__ __forceinline__ void dif_butterfly(double &ar, double &ai, double &br, double &bi, Cplx w) {
    const double ur = ar + br, ui = ai + bi, vr = ar - br, vi = ai - bi;
    ar = ur;
    ai = ui;
    br = vr * w.re - vi * w.im;
    bi = vr * w.im + vi * w.re;
}
// fft's butterfly (:218-222): v = b * w, a + v and a - v
__device__ __forceinline__ void dit_butterfly(double &ar, double &ai, double &br, double &bi, Cplx w) {
    const double vr = br * w.re - bi * w.im, vi = br * w.im + bi * w.re;
    const double ur = ar, ui = ai;
    ar = ur + vr;
    ai = ui + vi;
    br = ur - vr;
    bi = ui - vi;
}

// the stages len = 2^logt .. 2 of invfftlazy on 2^logt elements in LDS; begins and ends in a barrier
__device__ __forceinline__ void dif_stages(double *re, double *im, const CkksEncTables &tab, int logt) {
    __syncthreads();
    const int half = logt ? 1 << (logt - 1) : 0;
    for (int ll = logt; ll >= 1; --ll) {
        const int lenh = 1 << (ll - 1);
        for (int k = threadIdx.x; k < half; k += blockDim.x) {
            const int j = k & (lenh - 1), a = ((k >> (ll - 1)) << ll) + j, b = a + lenh;
            dif_butterfly(re[a], im[a], re[b], im[b], root_at(tab, dif_root_index(tab, ll, j)));
        }
        __syncthreads();
    }
}

// the stages len = 2 .. 2^logt of fft on 2^logt elements in LDS; begins and ends in a barrier
__device__ __forceinline__ void dit_stages(double *re, double *im, const CkksEncTables &tab, int logt) {
    __syncthreads();
    const int half = logt ? 1 << (logt - 1) : 0;
    for (int ll = 1; ll <= logt; ++ll) {
        const int lenh = 1 << (ll - 1);
        for (int k = threadIdx.x; k < half; k += blockDim.x) {
            const int j = k & (lenh - 1), a = ((k >> (ll - 1)) << ll) + j, b = a + lenh;
            dit_butterfly(re[a], im[a], re[b], im[b], root_at(tab, dit_root_index(tab, ll, j)));
        }
        __syncthreads();
    }
}

// Go's uint64(d) for 0 <= d < 2^64: the truncated integer.  Outside that domain Go's result depends on the machine; here it is the low 64
// bits of the truncated integer for a finite d >= 2^64, and 0 for a negative d, a NaN and an infinity.
__device__ __forceinline__ u64 f64_trunc_u64(double d) {
    if (!(d >= 1.0)) return 0;
    const u64 bits = (u64)__double_as_longlong(d);
    const int biased = (int)((bits >> 52) & 0x7ff);
    if (biased == 0x7ff) return 0;
    const u64 mant = (bits & ((1ull << 52) - 1)) | (1ull << 52);
    const int e = biased - 1075;                                  // d = mant * 2^e, e >= -52 as d >= 1
    if (e <= 0) return mant >> (-e);
    return e < 64 ? mant << e : 0;
}

// scaleUpVecExact (ckks/utils.go:51-98) for the coefficient x: its residue under every modulus of the level, stored at out[i * n]
__device__ __forceinline__ void scale_up_store(double x, const CkksScaleUp &S, u64 *out, int n) {
    const double y = S.scale * x;
    if (y > 1.8446744073709552e+19) {
        // the big.Float branch (:60-82), taken by positive coefficients only: at 53 bits the + 0.5 rounds away, Int() is the exact integer
        // mant * 2^e of the double, e >= 12; its residue is (mant mod q)(2^e mod q).  An infinity gives 0 (the reference's Int() of it is nil).
        const u64 bits = (u64)__double_as_longlong(y);
        const int biased = (int)((bits >> 52) & 0x7ff);
        const u64 mant = (bits & ((1ull << 52) - 1)) | (1ull << 52);
        for (int i = 0; i < S.limbs; ++i) {
            const u64 q = ld_const(&S.lp[i].q), uh = ld_const(&S.lp[i].bred_hi), ul = ld_const(&S.lp[i].bred_lo);
            u64 r = 0;
            if (biased != 0x7ff) {
                u64 p = 1 % q, b = 2 % q;
                for (int e = biased - 1075; e; e >>= 1) {
                    if (e & 1) p = bred(p, b, q, uh, ul);
                    b = bred(b, b, q, uh, ul);
                }
                r = bred(bred_add(mant, q, uh), p, q, uh, ul);
            }
            st_stream(out + (long long)i * n, r);
        }
        return;
    }
    // :85-93, in doubles: the + 0.5 rounds at and above 2^52 as the reference's does; a negative x with a zero remainder gives q, not 0
    const bool neg = x < 0;
    const u64 w = f64_trunc_u64((neg ? -y : y) + 0.5);
    for (int i = 0; i < S.limbs; ++i) {
        const u64 q = ld_const(&S.lp[i].q), r = bred_add(w, q, ld_const(&S.lp[i].bred_hi));
        st_stream(out + (long long)i * n, neg ? q - r : r);
    }
}

// Encode's tail (:96-105) for coefficient c of one plaintext: slot i's real part at i gap, its imaginary part at N / 2 + i gap, zeros between;
// `at(k)` is element k of invfftlazy's output before its bit reversal
template <class At>
__device__ __forceinline__ void encode_coefficient(int c, int n, int logslots, const CkksScaleUp &S, u64 *out, At at) {
    const int halfn = n >> 1, cc = c & (halfn - 1), gap = halfn >> logslots;
    if (cc & (gap - 1)) {
        for (int i = 0; i < S.limbs; ++i) st_stream(out + (long long)i * n + c, 0);
        return;
    }
    const Cplx v = at(bit_reverse_of((unsigned)(cc / gap), logslots));
    // values[i] /= complex(float64(N), 0) is Go's complex128div: ((re + im * 0) / N, (im - re * 0) / N), :200
    const double ns = (double)(1 << logslots);
    const double x = c < halfn ? (v.re + v.im * 0.0) / ns : (v.im - v.re * 0.0) / ns;
    scale_up_store(x, S, out + c, n);
}

__global__ __launch_bounds__(kCkksThreads) void ckks_encode_fused_kernel(CkksEncTables tab, const Cplx *values, int logslots, CkksScaleUp S) {
    extern __shared__ __align__(16) double ckks_lds[];
    const int slots = 1 << logslots, b = blockIdx.x;
    double *re = ckks_lds, *im = ckks_lds + slots;
    const double *v = (const double *)(values + (size_t)b * slots);
    for (int i = threadIdx.x; i < slots; i += kCkksThreads) {
        re[i] = v[2 * i];
        im[i] = v[2 * i + 1];
    }
    dif_stages(re, im, tab, logslots);
    u64 *out = S.out + (long long)b * S.out_stride;
    for (int c = threadIdx.x; c < tab.n; c += kCkksThreads)
        encode_coefficient(c, tab.n, logslots, S, out, [&](unsigned k) { return Cplx{re[k], im[k]}; });
}

__global__ __launch_bounds__(256) void ckks_dif_stage_kernel(CkksEncTables tab, const Cplx *src, Cplx *dst, int logslots, int ll) {
    const int k = blockIdx.x * 256 + threadIdx.x, half = 1 << (logslots - 1);
    if (k >= half) return;
    const size_t base = (size_t)blockIdx.y << logslots;
    const int lenh = 1 << (ll - 1), j = k & (lenh - 1), a = ((k >> (ll - 1)) << ll) + j, b = a + lenh;
    Cplx x = src[base + a], y = src[base + b];
    dif_butterfly(x.re, x.im, y.re, y.im, root_at(tab, dif_root_index(tab, ll, j)));
    dst[base + a] = x;
    dst[base + b] = y;
}

__global__ __launch_bounds__(kCkksThreads) void ckks_dif_tile_kernel(CkksEncTables tab, const Cplx *src, Cplx *dst, int logslots, int logt) {
    extern __shared__ __align__(16) double ckks_lds[];
    const int tile = 1 << logt;
    double *re = ckks_lds, *im = ckks_lds + tile;
    const size_t base = ((size_t)blockIdx.y << logslots) + ((size_t)blockIdx.x << logt);
    for (int i = threadIdx.x; i < tile; i += blockDim.x) {
        const Cplx v = src[base + i];
        re[i] = v.re;
        im[i] = v.im;
    }
    dif_stages(re, im, tab, logt);
    for (int i = threadIdx.x; i < tile; i += blockDim.x) dst[base + i] = Cplx{re[i], im[i]};
}

__global__ __launch_bounds__(256) void ckks_scale_up_kernel(CkksEncTables tab, const Cplx *src, int logslots, CkksScaleUp S) {
    const int c = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (c >= tab.n) return;
    const Cplx *v = src + ((size_t)b << logslots);
    encode_coefficient(c, tab.n, logslots, S, S.out + (long long)b * S.out_stride, [&](unsigned k) { return v[k]; });
}

// a >= b on `words` little-endian words
__device__ __forceinline__ bool words_geq(const u64 *a, const u64 *b, int words) {
    for (int w = words - 1; w >= 0; --w)
        if (a[w] != b[w]) return a[w] > b[w];
    return true;
}

// big.Float.SetInt(x).Float64() for the magnitude x on `words` words: round to nearest, ties to even, on the exact integer; +Inf from 2^1024
__device__ __forceinline__ double words_to_double(const u64 *x, int words) {
    int top = words - 1;
    while (top >= 0 && x[top] == 0) --top;
    if (top < 0) return 0.0;
    const int s = __clzll((long long)x[top]);
    int p = 64 * top + 63 - s;                                     // the leading bit
    const u64 below = top > 0 ? x[top - 1] : 0;
    const u64 window = s ? (x[top] << s) | (below >> (64 - s)) : x[top];   // the 64 bits from the leading one down
    bool sticky = (u64)(below << s) != 0 || (window & 0x3ff) != 0;
    for (int w = top - 2; w >= 0 && !sticky; --w) sticky = x[w] != 0;
    u64 mant = window >> 11;                                       // 53 bits
    const bool guard = (window >> 10) & 1;
    if (guard && (sticky || (mant & 1))) ++mant;
    if (mant >> 53) {
        mant >>= 1;
        ++p;
    }
    if (p >= 1024) return __longlong_as_double(0x7ff0000000000000ll);
    return __longlong_as_double((long long)(((u64)(p + 1023) << 52) | (mant & ((1ull << 52) - 1))));
}

__global__ __launch_bounds__(256) void ckks_crt_to_double_kernel(CkksEncTables tab, CkksCrt P, int logslots, double *dbuf) {
    const int idx = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y, slots = 1 << logslots;
    if (idx >= 2 * slots) return;
    const int n = tab.n, gap = (n >> 1) >> logslots, W = P.words;
    const int c = (idx >> logslots) * (n >> 1) + (idx & (slots - 1)) * gap;
    const u64 *row = P.pool + (long long)b * P.pool_stride + c;
    // x = sum_i ((a_i inv_i) mod q_i) (Q / q_i), below limbs * Q: W + 1 words
    u64 acc[kCkksCrtMaxWords + 1];
    for (int w = 0; w <= W; ++w) acc[w] = 0;
    for (int i = 0; i < P.limbs; ++i) {
        const u64 t = bred(ld_stream(row + (long long)i * n), ld_const(P.inv + i), ld_const(&P.lp[i].q), ld_const(&P.lp[i].bred_hi), ld_const(&P.lp[i].bred_lo));
        const u64 *h = P.qhat + (long long)i * P.qhat_stride;
        u64 carry = 0;
        for (int w = 0; w < W; ++w) {
            u64 hi, lo;
            mul_wide64(t, ld_const(h + w), hi, lo);
            const u64 s0 = acc[w] + lo, s1 = s0 + carry;
            acc[w] = s1;
            carry = hi + (u64)(s0 < lo) + (u64)(s1 < s0);          // t h + acc + carry <= 2^128 - 1: no overflow
        }
        acc[W] += carry;
    }
    // mod Q_level (:138), at most limbs - 1 subtractions
    u64 Q[kCkksCrtMaxWords], H[kCkksCrtMaxWords];
    for (int w = 0; w < W; ++w) {
        Q[w] = ld_const(P.Q + w);
        H[w] = ld_const(P.Qhalf + w);
    }
    while (acc[W] != 0 || words_geq(acc, Q, W)) {
        u64 borrow = 0;
        for (int w = 0; w < W; ++w) {
            const u64 d0 = acc[w] - Q[w], d1 = d0 - borrow;
            borrow = (u64)(acc[w] < Q[w]) | (u64)(d0 < borrow);
            acc[w] = d1;
        }
        acc[W] -= borrow;
    }
    // :139-141: minus Q from Q >> 1 up; the magnitude is Q - x
    const bool neg = words_geq(acc, H, W);
    if (neg) {
        u64 borrow = 0;
        for (int w = 0; w < W; ++w) {
            const u64 d0 = Q[w] - acc[w], d1 = d0 - borrow;
            borrow = (u64)(Q[w] < acc[w]) | (u64)(d0 < borrow);
            acc[w] = d1;
        }
    }
    const double mag = words_to_double(acc, W);
    dbuf[((size_t)b << (logslots + 1)) + idx] = (neg ? -mag : mag) / P.scale;         // scaleDown, ckks/utils.go:108-114
}

__global__ __launch_bounds__(kCkksThreads) void ckks_dit_tile_kernel(CkksEncTables tab, const double *dbuf, Cplx *dst, int logslots, int logt) {
    extern __shared__ __align__(16) double ckks_lds[];
    const int tile = 1 << logt, slots = 1 << logslots;
    double *re = ckks_lds, *im = ckks_lds + tile;
    const double *in = dbuf + ((size_t)blockIdx.y << (logslots + 1));
    const unsigned first = blockIdx.x << logt;
    for (int i = threadIdx.x; i < tile; i += blockDim.x) {
        const unsigned from = bit_reverse_of(first + i, logslots);                     // sliceBitReverseInPlaceComplex128, :209
        re[i] = in[from];
        im[i] = in[slots + from];
    }
    dit_stages(re, im, tab, logt);
    Cplx *out = dst + ((size_t)blockIdx.y << logslots) + first;
    for (int i = threadIdx.x; i < tile; i += blockDim.x) out[i] = Cplx{re[i], im[i]};
}

__global__ __launch_bounds__(256) void ckks_dit_stage_kernel(CkksEncTables tab, const Cplx *src, Cplx *dst, int logslots, int ll) {
    const int k = blockIdx.x * 256 + threadIdx.x, half = 1 << (logslots - 1);
    if (k >= half) return;
    const size_t base = (size_t)blockIdx.y << logslots;
    const int lenh = 1 << (ll - 1), j = k & (lenh - 1), a = ((k >> (ll - 1)) << ll) + j, b = a + lenh;
    Cplx x = src[base + a], y = src[base + b];
    dit_butterfly(x.re, x.im, y.re, y.im, root_at(tab, dit_root_index(tab, ll, j)));
    dst[base + a] = x;
    dst[base + b] = y;
}

// the dynamic-LDS limit is an attribute of the function on the CURRENT device: set once per device of the process
template <class Kernel>
hipError_t allow_lds(Kernel fn, std::atomic<bool> *configured) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::atomic<bool> &done = configured[dev >= 0 && dev < 64 ? dev : 0];
    if (done.load(std::memory_order_acquire)) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute((const void *)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(sizeof(Cplx) << kCkksFusedMaxLogSlots));
    if (e == hipSuccess) done.store(true, std::memory_order_release);
    return e;
}

bool tables_ok(const CkksEncTables &tab) { return tab.roots && tab.rot && tab.logn >= 1 && tab.logn <= 16 && tab.n == (1 << tab.logn); }
bool shape_ok(const CkksEncTables &tab, int logslots, int batch) { return tables_ok(tab) && logslots >= 0 && logslots <= tab.logn - 1 && batch <= 65535; }
// the threads of a workgroup that runs 2^logt elements in LDS: one butterfly each where that fills a wavefront
unsigned lds_threads(int logt) { return logt >= 11 ? kCkksThreads : (logt >= 7 ? 1u << (logt - 1) : 64u); }
unsigned blocks256(long long items) { return (unsigned)((items + 255) / 256); }

}  // namespace

hipError_t launch_ckks_encode_fused(const CkksEncTables &tab, const Cplx *values, int logslots, const CkksScaleUp &S, int batch, hipStream_t stream) {
    if (!shape_ok(tab, logslots, batch) || logslots > kCkksFusedMaxLogSlots || !values || !S.out || S.limbs < 1) return hipErrorInvalidValue;
    if (batch <= 0) return hipSuccess;
    static std::atomic<bool> configured[64];
    const hipError_t e = allow_lds(ckks_encode_fused_kernel, configured);
    if (e != hipSuccess) return e;
    return launch_kernel(ckks_encode_fused_kernel, dim3((unsigned)batch), dim3(kCkksThreads), sizeof(Cplx) << logslots, stream, tab, values, logslots, S);
}

hipError_t launch_ckks_dif_stage(const CkksEncTables &tab, const Cplx *src, Cplx *dst, int logslots, int loglen, int batch, hipStream_t stream) {
    if (!shape_ok(tab, logslots, batch) || loglen < 1 || loglen > logslots || !src || !dst) return hipErrorInvalidValue;
    if (batch <= 0) return hipSuccess;
    return launch_kernel(ckks_dif_stage_kernel, dim3(blocks256(1ll << (logslots - 1)), (unsigned)batch), dim3(256), 0, stream, tab, src, dst, logslots, loglen);
}

hipError_t launch_ckks_dif_tile(const CkksEncTables &tab, const Cplx *src, Cplx *dst, int logslots, int logtile, int batch, hipStream_t stream) {
    if (!shape_ok(tab, logslots, batch) || logtile < 0 || logtile > logslots || logtile > kCkksFusedMaxLogSlots || !src || !dst) return hipErrorInvalidValue;
    if (batch <= 0) return hipSuccess;
    static std::atomic<bool> configured[64];
    const hipError_t e = allow_lds(ckks_dif_tile_kernel, configured);
    if (e != hipSuccess) return e;
    return launch_kernel(ckks_dif_tile_kernel, dim3(1u << (logslots - logtile), (unsigned)batch), dim3(lds_threads(logtile)), sizeof(Cplx) << logtile, stream, tab, src, dst, logslots, logtile);
}

hipError_t launch_ckks_scale_up(const CkksEncTables &tab, const Cplx *src, int logslots, const CkksScaleUp &S, int batch, hipStream_t stream) {
    if (!shape_ok(tab, logslots, batch) || !src || !S.out || S.limbs < 1) return hipErrorInvalidValue;
    if (batch <= 0) return hipSuccess;
    return launch_kernel(ckks_scale_up_kernel, dim3(blocks256(tab.n), (unsigned)batch), dim3(256), 0, stream, tab, src, logslots, S);
}

hipError_t launch_ckks_crt_to_double(const CkksEncTables &tab, const CkksCrt &P, int logslots, double *dbuf, int batch, hipStream_t stream) {
    if (!shape_ok(tab, logslots, batch) || P.limbs < 1 || P.words < 1 || P.words > kCkksCrtMaxWords || P.qhat_stride < P.words || !P.pool || !dbuf)
        return hipErrorInvalidValue;
    if (batch <= 0) return hipSuccess;
    return launch_kernel(ckks_crt_to_double_kernel, dim3(blocks256(2ll << logslots), (unsigned)batch), dim3(256), 0, stream, tab, P, logslots, dbuf);
}

hipError_t launch_ckks_dit_tile(const CkksEncTables &tab, const double *dbuf, Cplx *dst, int logslots, int logtile, int batch, hipStream_t stream) {
    if (!shape_ok(tab, logslots, batch) || logtile < 0 || logtile > logslots || logtile > kCkksFusedMaxLogSlots || !dbuf || !dst) return hipErrorInvalidValue;
    if (batch <= 0) return hipSuccess;
    static std::atomic<bool> configured[64];
    const hipError_t e = allow_lds(ckks_dit_tile_kernel, configured);
    if (e != hipSuccess) return e;
    return launch_kernel(ckks_dit_tile_kernel, dim3(1u << (logslots - logtile), (unsigned)batch), dim3(lds_threads(logtile)), sizeof(Cplx) << logtile, stream, tab, dbuf, dst, logslots, logtile);
}

hipError_t launch_ckks_dit_stage(const CkksEncTables &tab, const Cplx *src, Cplx *dst, int logslots, int loglen, int batch, hipStream_t stream) {
    if (!shape_ok(tab, logslots, batch) || loglen < 1 || loglen > logslots || !src || !dst) return hipErrorInvalidValue;
    if (batch <= 0) return hipSuccess;
    return launch_kernel(ckks_dit_stage_kernel, dim3(blocks256(1ll << (logslots - 1)), (unsigned)batch), dim3(256), 0, stream, tab, src, dst, logslots, loglen);
}

}  // namespace lr
