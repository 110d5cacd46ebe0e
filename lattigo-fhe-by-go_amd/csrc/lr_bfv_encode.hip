// lr_bfv_encode.hip -- bfv.Encoder on the device (bfv/encoder.go:70-182): a batch of plaintexts per launch.
//
// Fused route: one workgroup per plaintext.  A plaintext modulus t < 2^31 fits 32-bit words and a whole transform over Z_t at
// N <= 2^15 fits one CU's LDS (4 N bytes <= 128 KiB of the 160), so encode reads the N slot values and writes the |Q| limbs, and
// decode reads SimpleScaler's one-limb row and writes the N slots; nothing in between touches memory.  The butterflies are the
// reference's (ring/ntt.go:53-139) with the powers of psi of the [t] context, out of Montgomery form and in 32-bit Shoup form
// (w, floor(w 2^32 / t)); every value is kept canonical in [0, t), so sums stay below 2 t < 2^32 and the Shoup remainder, which lies in
// [0, 2 t), is exact in 32 bits.  Canonical residues are unique: the outputs equal the reference's bit for bit.
//
// Composed route (every other shape: N = 2^16, t >= 2^31, N < 2^11): three streaming kernels around lr_intt / lr_ntt of the [t] context.
#include "lr_device.hpp"

#include <atomic>

namespace lr {

namespace {

constexpr int kEncThreads = 1024;

// the residue in [0, t) of slot value i of a plaintext: EncodeUint takes the value modulo t, EncodeInt maps a negative one to t - |c| mod t
__device__ __forceinline__ u64 slot_residue(const void *values, long long i, int is_signed, u64 t, u64 t_bred_hi) {
    if (!is_signed) return bred_add(((const u64 *)values)[i], t, t_bred_hi);
    const long long c = ((const long long *)values)[i];
    if (c >= 0) return bred_add((u64)c, t, t_bred_hi);
    const u64 r = bred_add(0 - (u64)c, t, t_bred_hi);
    return r ? t - r : 0;
}

// what a decoded slot is written as: DecodeInt subtracts t above t >> 1 (bfv/encoder.go:176-178)
__device__ __forceinline__ u64 slot_value(u64 v, int is_signed, u64 t) { return is_signed && v > (t >> 1) ? v - t : v; }

// x w mod t for any 32-bit x, w < t < 2^31
__device__ __forceinline__ u32 mul_shoup32(u32 x, Tw32 w, u32 t) {
    const u32 r = x * w.w - __umulhi(x, w.ws) * t;      // in [0, 2 t)
    return r >= t ? r - t : r;
}

// InvNTT's Gentleman-Sande stages (ring/ntt.go:89-139) on the N words in LDS, without the final scaling by N^-1; ends in a barrier
__device__ __forceinline__ void inverse_stages(u32 *lds, const Tw32 *tw, int logn, u32 t) {
    const int half = 1 << (logn - 1);
    for (int tlog = 0; tlog < logn; ++tlog) {
        const int span = 1 << tlog, h = half >> tlog;
        for (int k = threadIdx.x; k < half; k += kEncThreads) {
            const int i = k >> tlog, j = (i << (tlog + 1)) + (k & (span - 1));
            const Tw32 w = tw[h + i];
            const u32 U = lds[j], V = lds[j + span];
            const u32 s = U + V;
            lds[j] = s >= t ? s - t : s;
            lds[j + span] = mul_shoup32(U + t - V, w, t);
        }
        __syncthreads();
    }
}

// NTT's Cooley-Tukey stages (ring/ntt.go:53-87); canonical values, so the reference's final BRedAdd is the identity; ends in a barrier
__device__ __forceinline__ void forward_stages(u32 *lds, const Tw32 *tw, int logn, u32 t) {
    const int half = 1 << (logn - 1);
    for (int tlog = logn - 1; tlog >= 0; --tlog) {
        const int span = 1 << tlog, m = half >> tlog;
        for (int k = threadIdx.x; k < half; k += kEncThreads) {
            const int i = k >> tlog, j = (i << (tlog + 1)) + (k & (span - 1));
            const Tw32 w = tw[m + i];
            const u32 U = lds[j], V = mul_shoup32(lds[j + span], w, t);
            const u32 s = U + V, d = U + t - V;
            lds[j] = s >= t ? s - t : s;
            lds[j + span] = d >= t ? d - t : d;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(kEncThreads) void bfv_encode_fused_kernel(const EncodeLaunch L) {
    extern __shared__ __align__(16) u32 enc_lds[];
    const int n = L.tab.n, b = blockIdx.x;
    const u32 t = (u32)L.tab.t;
    const char *values = (const char *)L.values + (size_t)b * (size_t)L.n_values * sizeof(u64);
    for (int i = threadIdx.x; i < n; i += kEncThreads)
        enc_lds[L.tab.index[i]] = i < L.n_values ? (u32)slot_residue(values, i, L.is_signed, L.tab.t, L.tab.t_bred_hi) : 0u;
    __syncthreads();
    inverse_stages(enc_lds, L.tw_inv, L.tab.logn, t);
    u64 *out = L.out + (long long)b * L.out_stride;
    for (int j = threadIdx.x; j < n; j += kEncThreads) {
        const u64 m = mul_shoup32(enc_lds[j], L.n_inv, t);
        for (int i = 0; i < L.limbs; ++i)
            st_stream(out + (long long)i * n + j, mred(m, ld_const(L.delta_mont + i), ld_const(&L.lp[i].q), ld_const(&L.lp[i].qinv)));
    }
}

__global__ __launch_bounds__(kEncThreads) void bfv_decode_fused_kernel(const DecodeLaunch L) {
    extern __shared__ __align__(16) u32 enc_lds[];
    const int n = L.tab.n, b = blockIdx.x;
    const u64 *in = L.in + (long long)b * n;
    for (int j = threadIdx.x; j < n; j += kEncThreads) enc_lds[j] = (u32)ld_stream(in + j);
    __syncthreads();
    forward_stages(enc_lds, L.tw_fwd, L.tab.logn, (u32)L.tab.t);
    u64 *values = (u64 *)L.values + (long long)b * n;
    for (int i = threadIdx.x; i < n; i += kEncThreads) st_stream(values + i, slot_value(enc_lds[L.tab.index[i]], L.is_signed, L.tab.t));
}

__global__ __launch_bounds__(256) void bfv_slot_scatter_kernel(EncoderTables tab, const void *values, long long n_values, int is_signed, u64 *row) {
    const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (i >= tab.n) return;
    const char *v = (const char *)values + (size_t)b * (size_t)n_values * sizeof(u64);
    row[(long long)b * tab.n + tab.index[i]] = i < n_values ? slot_residue(v, i, is_signed, tab.t, tab.t_bred_hi) : 0;
}

__global__ __launch_bounds__(256) void bfv_lift_kernel(const u64 *row, int n, u64 *out, long long out_stride, int limbs, const LimbParams *lp,
                                                       const u64 *delta_mont) {
    const int j = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (j >= n) return;
    const u64 m = ld_stream(row + (long long)b * n + j);
    for (int i = 0; i < limbs; ++i)
        st_stream(out + (long long)b * out_stride + (long long)i * n + j, mred(m, ld_const(delta_mont + i), ld_const(&lp[i].q), ld_const(&lp[i].qinv)));
}

__global__ __launch_bounds__(256) void bfv_slot_gather_kernel(EncoderTables tab, const u64 *row, void *values, int is_signed) {
    const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (i >= tab.n) return;
    ((u64 *)values)[(long long)b * tab.n + i] = slot_value(row[(long long)b * tab.n + tab.index[i]], is_signed, tab.t);
}

// the dynamic-LDS limit is an attribute of the function on the CURRENT device: set once per device of the process
template <class Kernel>
hipError_t allow_lds(Kernel fn, std::atomic<bool> *configured) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::atomic<bool> &done = configured[dev >= 0 && dev < 64 ? dev : 0];
    if (done.load(std::memory_order_acquire)) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute((const void *)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(sizeof(u32) << 15));
    if (e == hipSuccess) done.store(true, std::memory_order_release);
    return e;
}

// the shapes the fused kernels are written for; the host decides the route with the same bounds (encoder_fused_shape, lr_bfv_encoder.cpp)
bool fused_shape(const EncoderTables &tab) {
    return tab.logn >= 11 && tab.logn <= 15 && tab.n == (1 << tab.logn) && tab.t >= 2 && tab.t < (1ull << 31);
}

}  // namespace

hipError_t launch_bfv_encode_fused(const EncodeLaunch &L, int batch, hipStream_t stream) {
    if (!fused_shape(L.tab) || L.n_values < 0 || L.n_values > L.tab.n || L.limbs < 1) return hipErrorInvalidValue;
    if (batch <= 0) return hipSuccess;
    static std::atomic<bool> configured[64];
    const hipError_t e = allow_lds(bfv_encode_fused_kernel, configured);
    if (e != hipSuccess) return e;
    return launch_kernel(bfv_encode_fused_kernel, dim3((unsigned)batch), dim3(kEncThreads), sizeof(u32) << L.tab.logn, stream, L);
}

hipError_t launch_bfv_decode_fused(const DecodeLaunch &L, int batch, hipStream_t stream) {
    if (!fused_shape(L.tab)) return hipErrorInvalidValue;
    if (batch <= 0) return hipSuccess;
    static std::atomic<bool> configured[64];
    const hipError_t e = allow_lds(bfv_decode_fused_kernel, configured);
    if (e != hipSuccess) return e;
    return launch_kernel(bfv_decode_fused_kernel, dim3((unsigned)batch), dim3(kEncThreads), sizeof(u32) << L.tab.logn, stream, L);
}

hipError_t launch_bfv_slot_scatter(const EncoderTables &tab, const void *values, long long n_values, int is_signed, u64 *row, int batch, hipStream_t stream) {
    if (n_values < 0 || n_values > tab.n || batch > 65535) return hipErrorInvalidValue;
    if (batch <= 0) return hipSuccess;
    return launch_kernel(bfv_slot_scatter_kernel, dim3((unsigned)((tab.n + 255) / 256), (unsigned)batch), dim3(256), 0, stream, tab, values, n_values, is_signed, row);
}

hipError_t launch_bfv_lift(const u64 *row, int n, u64 *out, long long out_stride, int limbs, const LimbParams *lp, const u64 *delta_mont, int batch,
                           hipStream_t stream) {
    if (batch > 65535) return hipErrorInvalidValue;
    if (batch <= 0) return hipSuccess;
    return launch_kernel(bfv_lift_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)batch), dim3(256), 0, stream, row, n, out, out_stride, limbs, lp, delta_mont);
}

hipError_t launch_bfv_slot_gather(const EncoderTables &tab, const u64 *row, void *values, int is_signed, int batch, hipStream_t stream) {
    if (batch > 65535) return hipErrorInvalidValue;
    if (batch <= 0) return hipSuccess;
    return launch_kernel(bfv_slot_gather_kernel, dim3((unsigned)((tab.n + 255) / 256), (unsigned)batch), dim3(256), 0, stream, tab, row, values, is_signed);
}

}  // namespace lr
