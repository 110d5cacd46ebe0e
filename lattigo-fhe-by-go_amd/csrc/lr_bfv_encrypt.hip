// lr_bfv_encrypt.hip -- the kernels of the BFV encryptor (lr_bfv_encryptor.cpp): the samplers' compact decisions expanded into limbs, and
// the sk product.  Streaming passes (lr_stream.hpp), batch on blockIdx.z.
#include "lr_stream.hpp"

namespace lr {

__global__ __launch_bounds__(256) void bfv_ternary_kernel(TernaryLaunch L) {
    const int limb = blockIdx.y;
    const long long b = blockIdx.z;
    const u64 one = L.one.v[limb], minus_one = L.minus_one.v[limb];
    const long long plane = (long long)(L.n >> 3);
    const unsigned char *pc = L.coeff_bits + b * plane, *ps = L.sign_bits + b * plane;
    ulonglong2 *po = row_out(L.out, b, L.out_stride, (long long)limb * L.n);
    const int pairs = L.n >> 1;
    LR_FOR_PAIRS(e, pairs) st_stream(po + e, ternary_pair(pc, ps, e, one, minus_one));
}

hipError_t launch_bfv_ternary(const TernaryLaunch &L, int limbs, int batch, hipStream_t stream) {
    if (const LaunchVerdict v = launch_verdict(L, limbs, batch)) return verdict_error(v);
    return launch_kernel(bfv_ternary_kernel, pair_grid(L.n, (unsigned)limbs, (unsigned)batch), dim3(256), 0, stream, L);
}

// grid y = component * limbs + limb
template <bool ADD>
__global__ __launch_bounds__(256) void bfv_noise_kernel(NoiseLaunch L, int limbs) {
    const int comp = blockIdx.y / limbs, limb = blockIdx.y - comp * limbs;
    const long long b = blockIdx.z;
    const u64 q = L.lp[limb].q;
    const long long row = (long long)limb * L.n;
    const unsigned char *pe = L.e[comp] + b * (long long)L.n;      // (byte loads: a caller's device pointer may have any alignment)
    const ulonglong2 *px = ADD ? row_in(L.x[comp], b, L.x_stride[comp], row) : nullptr;
    const ulonglong2 *pp = ADD && L.plus[comp] ? row_in(L.plus[comp], b, L.plus_stride[comp], row) : nullptr;
    ulonglong2 *po = row_out(L.out[comp], b, L.out_stride[comp], row);
    const int pairs = L.n >> 1;
    LR_FOR_PAIRS(e, pairs) {
        ulonglong2 r = make_ulonglong2(noise_residue(pe[2 * e], q), noise_residue(pe[2 * e + 1], q));
        if constexpr (ADD) {
            r = add2(ld_stream(px + e), r, q);
            if (pp) r = add2(r, ld_stream(pp + e), q);
        }
        st_stream(po + e, r);
    }
}

hipError_t launch_bfv_noise(const NoiseLaunch &L, int comps, int limbs, int batch, hipStream_t stream) {
    if (const LaunchVerdict v = launch_verdict(L, comps, limbs, batch)) return verdict_error(v);
    const dim3 grid = pair_grid(L.n, (unsigned)(comps * limbs), (unsigned)batch);
    return L.add ? launch_kernel(bfv_noise_kernel<true>, grid, dim3(256), 0, stream, L, limbs)
                 : launch_kernel(bfv_noise_kernel<false>, grid, dim3(256), 0, stream, L, limbs);
}

__global__ __launch_bounds__(256) void bfv_negmul_kernel(NegMulLaunch L) {
    const int limb = blockIdx.y;
    const long long b = blockIdx.z;
    const LimbParams lp = L.lp[limb];
    const u64 q = lp.q;
    const long long row = (long long)limb * L.n;
    const ulonglong2 *pa = row_in(L.a, b, L.a_stride, row), *pb = row_in(L.b, b, L.b_stride, row);
    ulonglong2 *po = row_out(L.out, b, L.out_stride, row);
    const int pairs = L.n >> 1;
    LR_FOR_PAIRS(e, pairs) {
        const ulonglong2 x = ld_stream(pa + e), y = ld_shared(pb, L.b_stride, e);
        st_stream(po + e, neg2(mul2(x, y, q, lp.qinv), q));
    }
}

hipError_t launch_bfv_negmul(const NegMulLaunch &L, int limbs, int batch, hipStream_t stream) {
    if (const LaunchVerdict v = launch_verdict(L, limbs, batch)) return verdict_error(v);
    return launch_kernel(bfv_negmul_kernel, pair_grid(L.n, (unsigned)limbs, (unsigned)batch), dim3(256), 0, stream, L);
}

}  // namespace lr
