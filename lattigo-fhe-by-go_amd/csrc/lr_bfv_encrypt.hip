// lr_bfv_encrypt.hip -- the kernels of the BFV encryptor (lr_bfv_encryptor.cpp): the samplers' compact decisions expanded into limbs, and
// the sk product.  Streaming kernels in the manner of lr_ewise.hip: 16 B per lane per access to poly data, two coefficients per lane,
// limb on blockIdx.y (per-modulus constants wave-uniform), batch on blockIdx.z, a grid-stride loop over coefficient pairs.
#include "lr_device.hpp"

namespace lr {

namespace {

dim3 pair_grid(int n, unsigned y, unsigned z) {
    int gx = ((n >> 1) + 255) / 256;
    if (gx > 64) gx = 64;
    if (gx < 1) gx = 1;
    return dim3((unsigned)gx, y, z);
}

}  // namespace

// Pair e holds coefficients 2e and 2e + 1: both bits of a plane sit in byte e >> 2 at bit 2 (e & 3), so a lane takes its two decisions
// from one byte load per plane (four neighbouring lanes share the byte) and a wave's 16-byte stores stay contiguous.
__global__ __launch_bounds__(256) void bfv_ternary_kernel(TernaryLaunch L) {
    const int limb = blockIdx.y;
    const long long b = blockIdx.z;
    const u64 one = L.one.v[limb], minus_one = L.minus_one.v[limb];
    const long long plane = (long long)(L.n >> 3);
    const unsigned char *pc = L.coeff_bits + b * plane, *ps = L.sign_bits + b * plane;
    ulonglong2 *po = reinterpret_cast<ulonglong2 *>(L.out + b * L.out_stride + (long long)limb * L.n);
    const int pairs = L.n >> 1;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < pairs; e += gridDim.x * 256) {
        const unsigned sh = (unsigned)(e & 3) * 2;
        const unsigned c = (unsigned)pc[e >> 2] >> sh, s = (unsigned)ps[e >> 2] >> sh;
        // index 0 -> 0, 1 (coeff, sign 0) -> MForm(1), 2 (coeff, sign 1) -> MForm(q - 1)
        const u64 v0 = (c & 1) ? ((s & 1) ? minus_one : one) : 0;
        const u64 v1 = (c & 2) ? ((s & 2) ? minus_one : one) : 0;
        st_stream(po + e, make_ulonglong2(v0, v1));
    }
}

hipError_t launch_bfv_ternary(const TernaryLaunch &L, int limbs, int batch, hipStream_t stream) {
    if (limbs <= 0 || batch <= 0) return hipSuccess;
    if (L.n < 8 || limbs > kMaxLimbs) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(bfv_ternary_kernel, pair_grid(L.n, (unsigned)limbs, (unsigned)batch), dim3(256), 0, stream, L);
    return hipGetLastError();
}

LR_D u64 noise_residue(unsigned byte, u64 q) {
    const u64 c = byte & 127u;
    return (byte & 128u) ? c : q - c;
}

// grid y = component * limbs + limb
template <bool ADD>
__global__ __launch_bounds__(256) void bfv_noise_kernel(NoiseLaunch L, int limbs) {
    const int comp = blockIdx.y / limbs, limb = blockIdx.y - comp * limbs;
    const long long b = blockIdx.z;
    const u64 q = L.lp[limb].q;
    const long long row = (long long)limb * L.n;
    const unsigned char *pe = L.e[comp] + b * (long long)L.n;      // (byte loads: a caller's device pointer may have any alignment)
    const ulonglong2 *px = ADD ? reinterpret_cast<const ulonglong2 *>(L.x[comp] + b * L.x_stride[comp] + row) : nullptr;
    const ulonglong2 *pp = ADD && L.plus[comp] ? reinterpret_cast<const ulonglong2 *>(L.plus[comp] + b * L.plus_stride[comp] + row) : nullptr;
    ulonglong2 *po = reinterpret_cast<ulonglong2 *>(L.out[comp] + b * L.out_stride[comp] + row);
    const int pairs = L.n >> 1;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < pairs; e += gridDim.x * 256) {
        ulonglong2 r = make_ulonglong2(noise_residue(pe[2 * e], q), noise_residue(pe[2 * e + 1], q));
        if constexpr (ADD) {
            const ulonglong2 x = ld_stream(px + e);
            r.x = cred(x.x + r.x, q);
            r.y = cred(x.y + r.y, q);
            if (pp) {
                const ulonglong2 p = ld_stream(pp + e);
                r.x = cred(r.x + p.x, q);
                r.y = cred(r.y + p.y, q);
            }
        }
        st_stream(po + e, r);
    }
}

hipError_t launch_bfv_noise(const NoiseLaunch &L, int comps, int limbs, int batch, hipStream_t stream) {
    if (limbs <= 0 || batch <= 0 || comps <= 0) return hipSuccess;
    if (comps > 2 || L.n < 2 || (long long)comps * limbs > 65535) return hipErrorInvalidValue;
    const dim3 grid = pair_grid(L.n, (unsigned)(comps * limbs), (unsigned)batch);
    (void)hipGetLastError();
    if (L.add) hipLaunchKernelGGL(bfv_noise_kernel<true>, grid, dim3(256), 0, stream, L, limbs);
    else hipLaunchKernelGGL(bfv_noise_kernel<false>, grid, dim3(256), 0, stream, L, limbs);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void bfv_negmul_kernel(NegMulLaunch L) {
    const int limb = blockIdx.y;
    const long long b = blockIdx.z;
    const LimbParams lp = L.lp[limb];
    const u64 q = lp.q;
    const long long row = (long long)limb * L.n;
    const ulonglong2 *pa = reinterpret_cast<const ulonglong2 *>(L.a + b * L.a_stride + row);
    const ulonglong2 *pb = reinterpret_cast<const ulonglong2 *>(L.b + b * L.b_stride + row);
    ulonglong2 *po = reinterpret_cast<ulonglong2 *>(L.out + b * L.out_stride + row);
    const int pairs = L.n >> 1;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < pairs; e += gridDim.x * 256) {
        const ulonglong2 x = ld_stream(pa + e);
        const ulonglong2 y = L.b_stride ? ld_stream(pb + e) : pb[e];   // (a key shared by the batch: through the caches)
        st_stream(po + e, make_ulonglong2(q - mred(x.x, y.x, q, lp.qinv), q - mred(x.y, y.y, q, lp.qinv)));
    }
}

hipError_t launch_bfv_negmul(const NegMulLaunch &L, int limbs, int batch, hipStream_t stream) {
    if (limbs <= 0 || batch <= 0) return hipSuccess;
    if (L.n < 2) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(bfv_negmul_kernel, pair_grid(L.n, (unsigned)limbs, (unsigned)batch), dim3(256), 0, stream, L);
    return hipGetLastError();
}

}  // namespace lr
