// lr_bfv_chain.cpp -- C ABI: chains of BFV rotations as one call each on an lr_ckks_plan: lr_bfv_inner_sum (bfv/evaluator.go:691-708) and
// lr_bfv_rotate_chain (rotateColumnsPow2 :637-666; InnerSum is its accumulating form with the row rotation at the end).  A chain over a
// state (a0, a1) takes, per step i with Galois element g_i and key K_i, bfv.evaluator.permute (:711-733):
//   (e0, e1) = (Permute(a0, g_i), Permute(a1, g_i))       (p0, p1) = switchKeys(e1, K_i)       (r0, r1) = (CRed(e0 + p0), p1)
//   replace:     (a0, a1) <- (r0, r1)                          accumulate:  (a0, a1) <- (CRed(r0 + a0), CRed(r1 + a1))
// The key switch is bfv_switch_keys_core as every BFV pipeline calls it.  Around it the fused route makes ONE pass per step
// (launch_bfv_chain_step, lr_ewise.hip), which also writes the next step's key-switch input; the composed route makes the reference's
// own calls (launch_permute x2, LR_ADD, and LR_ADD x2 when accumulating).  Same bits on both.
// The unit's name keeps it out of the lr_abi_*.cpp set (its launcher has a stand-in of its own under tests/cpp).
#include "lr_host.hpp"

namespace lr_host {
namespace {

enum class ChainRoute { Fused, Composed };
// THE route decision of a chain: the fused step pass where a row fits the LDS, unless the plan or its context asks for
// the call-by-call shape (lr_options::no_epilogue, as lr_setup reads it).  One regime is measured the other way: the
// replace chain of ONE ciphertext at N = 2^14.  Its step pass is 2 |Q| workgroups that each walk a whole row twice, while lr_bfv_rotate's
// launches for a single ciphertext -- both Permutes as one launch, the key switch straight into the destination, one Add -- leave nothing
// for the pass to save but that Add: 1599 us against 1573 us for 13 steps at PN14QP438.  From two ciphertexts on the pass wins everywhere.
ChainRoute chain_route(const lr_ckks_plan *pl, int batch, bool accumulate) {
    const int logn = (int)pl->cQ->h.logN;
    if (pl->opt.no_epilogue || pl->cQ->opt.no_epilogue) return ChainRoute::Composed;
    if (!lr::lds_row_degree(logn) || batch > 65535) return ChainRoute::Composed;
    if (!accumulate && batch == 1 && logn == 14 && !pl->opt.no_pair) return ChainRoute::Composed;
    return ChainRoute::Fused;
}

// a component of the state: the caller's poly or one half of a pool pair
struct Comp {
    u64 *d;
    long long stride;
};

int permute_coeff(lr_context *cQ, int L1, int batch, const u64 *in, long long in_stride, u64 *out, long long out_stride, u64 gen) {
    GaloisLaunch G;
    G.n = (int)cQ->h.N;
    G.logn = (int)cQ->h.logN;
    G.ntt_domain = 0;
    G.gen = gen & ((cQ->h.N << 1) - 1);
    G.lp = cQ->d_lp;
    G.in = in; G.in_stride = in_stride; G.out = out; G.out_stride = out_stride;
    LR_HIP(launch_permute(G, L1, batch, cQ->stream));
    return LR_OK;
}

// the shared checks of the two entry points, after their own argument checks: shapes
int check_chain_shapes(const lr_ckks_plan *pl, const lr_poly *c0, const lr_poly *c1, const lr_poly *o0, const lr_poly *o1) {
    const int level = pl->cQ->h.L() - 1, batch = c0->batch;
    if (batch > pl->max_batch) return fail(LR_ERR_SHAPE, "batch exceeds the plan's max_batch");
    for (const lr_poly *p : {c0, c1, o0, o1}) LR_TRY(check_ct(pl, level, p, batch));
    if (pl->cQ->h.N < 2 || pl->cQ->h.logN > 31) return fail(LR_ERR_UNSUPPORTED, "ring degree");
    return LR_OK;
}

// the chain itself; every argument checked
int chain_core(lr_ckks_plan *pl, const lr_poly *c0, const lr_poly *c1, int n_steps, const u64 *gens, const lr_poly *const *keys, bool accumulate,
               lr_poly *o0, lr_poly *o1) {
    lr_context *cQ = pl->cQ;
    const int batch = c0->batch, L1 = cQ->h.L(), n = (int)cQ->h.N;
    const long long s = (long long)L1 * n;
    LR_TRY(same_stream(pl->cQ, pl->cP));
    LR_HIP(hipSetDevice(pl->device));
    const bool fused = chain_route(pl, batch, accumulate) == ChainRoute::Fused;
    for (Pool *p : {&pl->bfvP, &pl->chainP}) LR_TRY(p->ensure(cQ, (size_t)2 * batch * s));
    for (Pool *p : {&pl->c0, &pl->c2x}) LR_TRY(p->ensure(cQ, (size_t)batch * s));
    u64 *const pair[2] = {pl->bfvP.d, pl->chainP.d};       // each [2][batch][|Q|][N]: back to back, so the key switch's tail takes both halves at once
    auto copy = [&](const u64 *in, long long in_stride, u64 *out, long long out_stride) -> int {
        return in == out ? (int)LR_OK : run_ewise(cQ, LR_COPY, L1, batch, in, in_stride, nullptr, 0, out, out_stride, nullptr);
    };
    Comp a[2] = {{c0->d, c0->stride()}, {c1->d, c1->stride()}};
    const Comp out[2] = {{o0->d, o0->stride()}, {o1->d, o1->stride()}};
    int next = 0;      // the pool pair the next key switch accumulates into; the state is never there
    if (out[0].d == a[1].d || out[1].d == a[0].d) {
        // an output over the OTHER component's input: every pass here is local to its own component's row, so the state starts as a copy
        for (int k = 0; k < 2; ++k) {
            u64 *dst = pair[1] + (long long)k * batch * s;
            LR_TRY(copy(a[k].d, a[k].stride, dst, s));
            a[k] = {dst, s};
        }
    }
    if (n_steps == 0) {
        for (int k = 0; k < 2; ++k) LR_TRY(copy(a[k].d, a[k].stride, out[k].d, out[k].stride));
        return LR_OK;
    }
    if (fused) LR_TRY(permute_coeff(cQ, L1, batch, a[1].d, a[1].stride, pl->c2x.d, s, gens[0]));      // :724 of the first step; the later ones come out of the step pass
    for (int i = 0; i < n_steps; ++i) {
        const bool last = i == n_steps - 1;
        u64 *const p[2] = {pair[next], pair[next] + (long long)batch * s};
        const Comp dst[2] = {last ? out[0] : Comp{p[0], s}, last ? out[1] : Comp{p[1], s}};
        if (fused) {
            LR_TRY(bfv_switch_keys_core(pl, batch, pl->c2x.d, s, keys[i], {{p[0], p[1]}, {s, s}}));       // :729
            BfvChainStepLaunch S;
            S.a0 = a[0].d; S.a0_stride = a[0].stride; S.a1 = a[1].d; S.a1_stride = a[1].stride;
            S.p0 = p[0]; S.p1 = p[1]; S.p_stride = s;
            S.out0 = dst[0].d; S.out0_stride = dst[0].stride; S.out1 = dst[1].d; S.out1_stride = dst[1].stride;
            S.cx_next = last ? nullptr : pl->c2x.d; S.cx_stride = s;
            S.n = n; S.logn = (int)cQ->h.logN;
            S.ginv = galois_inverse(gens[i], n);
            S.ginv_next = last ? 1u : galois_inverse(gens[i + 1], n);
            S.accumulate = accumulate ? 1 : 0;
            S.lp = cQ->d_lp;
            LR_HIP(launch_bfv_chain_step(S, L1, batch, cQ->stream));
        } else {
            const ComponentPair ins = component_pair(a[0].d, a[0].stride, a[1].d, a[1].stride, batch);
            if (batch == 1 && !pl->opt.no_pair && ins) {
                // one ciphertext: both components in one launch, the strides are the distances between them (see lr_bfv_rotate)
                LR_TRY(permute_coeff(cQ, L1, 2, a[0].d, ins.stride, pl->c0.d, component_distance(pl->c0.d, pl->c2x.d), gens[i]));   // :723-724
            } else {
                LR_TRY(permute_coeff(cQ, L1, batch, a[0].d, a[0].stride, pl->c0.d, s, gens[i]));          // :723
                LR_TRY(permute_coeff(cQ, L1, batch, a[1].d, a[1].stride, pl->c2x.d, s, gens[i]));         // :724
            }
            if (accumulate) {
                LR_TRY(bfv_switch_keys_core(pl, batch, pl->c2x.d, s, keys[i], {{p[0], p[1]}, {s, s}}));                            // :729
                LR_TRY(run_ewise(cQ, LR_ADD, L1, batch, pl->c0.d, s, p[0], s, p[0], s, nullptr));                                  // :731
                LR_TRY(run_ewise(cQ, LR_ADD, L1, batch, p[0], s, a[0].d, a[0].stride, dst[0].d, dst[0].stride, nullptr));          // InnerSum :703 / :707
                LR_TRY(run_ewise(cQ, LR_ADD, L1, batch, p[1], s, a[1].d, a[1].stride, dst[1].d, dst[1].stride, nullptr));
            } else {
                // the state is dead once it is permuted: the key switch accumulates straight into the step's destination (p1 lands in
                // out1, :732), as in lr_bfv_rotate
                LR_TRY(bfv_switch_keys_core(pl, batch, pl->c2x.d, s, keys[i], {{dst[0].d, dst[1].d}, {dst[0].stride, dst[1].stride}}));   // :729
                LR_TRY(run_ewise(cQ, LR_ADD, L1, batch, pl->c0.d, s, dst[0].d, dst[0].stride, dst[0].d, dst[0].stride, nullptr));  // :731
            }
        }
        a[0] = dst[0];
        a[1] = dst[1];
        next ^= 1;
    }
    return LR_OK;
}

}  // namespace
}  // namespace lr_host

extern "C" int lr_bfv_rotate_chain(lr_ckks_plan *pl, const lr_poly *c0, const lr_poly *c1, int n_steps, const uint64_t *gens,
                                   const lr_poly *const *keys, int accumulate, lr_poly *o0, lr_poly *o1) {
    return guarded([&]() -> int {
    if (!pl || !c0 || !c1 || !o0 || !o1) return fail(LR_ERR_ARG, "null argument");
    if (n_steps < 0) return fail(LR_ERR_ARG, "negative step count");
    if (n_steps > 0 && (!gens || !keys)) return fail(LR_ERR_ARG, "null argument");
    for (int i = 0; i < n_steps; ++i) {
        if (!keys[i]) return fail(LR_ERR_ARG, "null argument");
        if (!(gens[i] & 1)) return fail(LR_ERR_ARG, "bfv rotate chain: a Galois element must be odd");
    }
    if (o0 == o1 || o0->d == o1->d) return fail(LR_ERR_ARG, "bfv rotate chain: the two output polys must be distinct");
    LR_TRY(check_chain_shapes(pl, c0, c1, o0, o1));
    return chain_core(pl, c0, c1, n_steps, gens, keys, accumulate != 0, o0, o1);
    });
}

extern "C" int lr_bfv_inner_sum(lr_ckks_plan *pl, const lr_poly *c0, const lr_poly *c1, int n_col_keys, const lr_poly *const *col_keys,
                                const lr_poly *row_key, lr_poly *o0, lr_poly *o1) {
    return guarded([&]() -> int {
    if (!pl || !c0 || !c1 || !row_key || !o0 || !o1 || (n_col_keys > 0 && !col_keys)) return fail(LR_ERR_ARG, "null argument");
    for (int i = 0; i < n_col_keys; ++i)
        if (!col_keys[i]) return fail(LR_ERR_ARG, "null argument");
    if (o0 == o1 || o0->d == o1->d) return fail(LR_ERR_ARG, "bfv inner sum: the two output polys must be distinct");
    const int logn = (int)pl->cQ->h.logN;
    if (n_col_keys != logn - 1) return fail(LR_ERR_ARG, "bfv inner sum: needs the keys of the left rotations by 2^i, i = 0 .. log2(N) - 2");
    LR_TRY(check_chain_shapes(pl, c0, c1, o0, o1));
    // galElRotColLeft[2^i] = 5^(2^i) mod 2N (:701-702), then galElRotRow = 2N - 1 (:706)
    const u64 mask = (pl->cQ->h.N << 1) - 1;
    std::vector<u64> gens;
    std::vector<const lr_poly *> keys;
    u64 g = 5 & mask;
    for (int i = 0; i < n_col_keys; ++i, g = (g * g) & mask) {
        gens.push_back(g);
        keys.push_back(col_keys[i]);
    }
    gens.push_back(mask);
    keys.push_back(row_key);
    return chain_core(pl, c0, c1, (int)gens.size(), gens.data(), keys.data(), true, o0, o1);
    });
}
