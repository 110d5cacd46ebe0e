// lr_abi_bfv_eval.cpp -- C ABI: the BFV evaluator's key-switch pipelines on an lr_ckks_plan, over bfv_switch_keys_core / _grouped
// (lr_abi_ckks.cpp): lr_bfv_switch_keys, lr_bfv_relinearize, lr_bfv_rotate, the rotation chains lr_bfv_rotate_chain / lr_bfv_inner_sum and
// lr_bfv_relinearize_deg.  Two steps carry them, each written once:
//   bfv_rotate_step          bfv.evaluator.permute (bfv/evaluator.go:711-733): lr_bfv_rotate, and each replace step of a composed chain
//   bfv_relin_composed_step  one degree of Relinearize (:489-495): lr_bfv_relinearize, and each degree of lr_bfv_relinearize_deg's composed route
// A chain over a state (a0, a1) takes, per step i with Galois element g_i and key K_i:
//   (e0, e1) = (Permute(a0, g_i), Permute(a1, g_i))       (p0, p1) = switchKeys(e1, K_i)       (r0, r1) = (CRed(e0 + p0), p1)
//   replace:     (a0, a1) <- (r0, r1)                          accumulate:  (a0, a1) <- (CRed(r0 + a0), CRed(r1 + a1))
// Around the key switch the fused route makes ONE pass per step (launch_bfv_chain_step, lr_ewise.hip), which also writes the next step's
// key-switch input; the composed route makes the reference's own calls (launch_permute x2, LR_ADD, and LR_ADD x2 when accumulating).
// Relinearize of degree d is
//   (a0, a1) = (ct[0], ct[1]);   for deg = d .. 2:  (p0, p1) = switchKeys(ct[deg], evakey[deg - 2]);  a0 = CRed(a0 + p0);  a1 = CRed(a1 + p1)
// The d - 1 key switches share no data.  The composed route runs them one after the other; the merged route runs G of them as ONE key switch
// over G * batch members with one key per group (bfv_switch_keys_grouped) and adds the pass's G results to the running pair in one launch
// (launch_bfv_relin_fold, lr_ewise.hip), in the reference's order.  Same bits on every route.
#include "lr_host.hpp"

namespace lr_host {
namespace {

// words of one poly over Q
long long poly_words(const lr_context *cQ) { return (long long)cQ->h.L() * (long long)cQ->h.N; }

int check_permute_degree(const lr_context *cQ) {
    if (cQ->h.N < 2 || cQ->h.logN > 31) return fail(LR_ERR_UNSUPPORTED, "ring degree");
    return LR_OK;
}

// Context.Permute of both components (:723-724) into pl->c0 / pl->c2x, which hold `batch` polys each
int bfv_permute_pair(lr_ckks_plan *pl, int batch, const Comp &a0, const Comp &a1, u64 gen) {
    lr_context *cQ = pl->cQ;
    const int L1 = cQ->h.L();
    const long long s = poly_words(cQ);
    const ComponentPair ins = component_pair(a0.d, a0.stride, a1.d, a1.stride, batch);
    if (batch == 1 && !pl->opt.no_pair && ins)
        // one ciphertext: both components in one launch, the strides are the distances between them (see ckks_rotate_step)
        return run_permute(cQ, false, L1, 2, a0.d, ins.stride, pl->c0.d, component_distance(pl->c0.d, pl->c2x.d), gen);   // :723-724
    LR_TRY(run_permute(cQ, false, L1, batch, a0.d, a0.stride, pl->c0.d, s, gen));        // :723
    return run_permute(cQ, false, L1, batch, a1.d, a1.stride, pl->c2x.d, s, gen);        // :724
}

// bfv.evaluator.permute (:711-733): Permute of both components, switchKeys of the second (:729), Add and Copy (:731-732).  The key switch
// accumulates straight into the destination (the reference's keyswitchpool[2], [3] and its Copy are the same values: p1 lands in dst1),
// which may be the input (the reference's polypool branch, :717-721).
int bfv_rotate_step(lr_ckks_plan *pl, int batch, const Comp &a0, const Comp &a1, u64 gen, const lr_poly *key, const Comp &dst0, const Comp &dst1) {
    lr_context *cQ = pl->cQ;
    const long long s = poly_words(cQ);
    LR_TRY(bfv_permute_pair(pl, batch, a0, a1, gen));
    LR_TRY(bfv_switch_keys_core(pl, batch, pl->c2x.d, s, key, {{dst0.d, dst1.d}, {dst0.stride, dst1.stride}}));       // :729
    return run_ewise(cQ, LR_ADD, cQ->h.L(), batch, pl->c0.d, s, dst0.d, dst0.stride, dst0.d, dst0.stride, nullptr);   // :731
}

// :494-495: out = (a0 + p0, a1 + p1).  One ciphertext's two additions are one launch over two "polys" at the distances between the
// components, where the operands allow it: no output over the other component's operand, the two addends back to back.
int bfv_add_pair(lr_ckks_plan *pl, int batch, const Comp (&a)[2], const u64 *p0, const u64 *p1, long long p_stride, const Comp (&out)[2]) {
    lr_context *cQ = pl->cQ;
    const int L1 = cQ->h.L();
    const ComponentPair ins = component_pair(a[0].d, a[0].stride, a[1].d, a[1].stride, batch);
    const ComponentPair outs = component_pair(out[0].d, out[0].stride, out[1].d, out[1].stride, batch);
    if (batch == 1 && !pl->opt.no_pair && ins && outs && out[0].d != a[1].d && out[1].d != a[0].d && p1 == p0 + p_stride)
        return run_ewise(cQ, LR_ADD, L1, 2, a[0].d, ins.stride, p0, p_stride, out[0].d, outs.stride, nullptr);          // :494-495
    LR_TRY(run_ewise(cQ, LR_ADD, L1, batch, a[0].d, a[0].stride, p0, p_stride, out[0].d, out[0].stride, nullptr));      // :494
    return run_ewise(cQ, LR_ADD, L1, batch, a[1].d, a[1].stride, p1, p_stride, out[1].d, out[1].stride, nullptr);       // :495
}

// one degree of Relinearize the reference's way: out = (a0 + p0, a1 + p1) with (p0, p1) = switchKeys(cx, evk) in pl->bfvP
int bfv_relin_composed_step(lr_ckks_plan *pl, int batch, const Comp &cx, const lr_poly *evk, const Comp (&a)[2], const Comp (&out)[2]) {
    lr_context *cQ = pl->cQ;
    const long long s = poly_words(cQ);
    LR_TRY(pl->bfvP.ensure(cQ, (size_t)2 * batch * s));         // keyswitchpool[2], [3] (:489-490)
    u64 *const p0 = pl->bfvP.d, *const p1 = pl->bfvP.d + (long long)batch * s;
    LR_TRY(bfv_switch_keys_core(pl, batch, cx.d, cx.stride, evk, {{p0, p1}, {s, s}}));      // :493
    return bfv_add_pair(pl, batch, a, p0, p1, s, out);
}

enum class ChainRoute { Fused, Composed };
// THE route decision of a chain: the fused step pass where a row fits the LDS, unless the plan or its context asks for
// the call-by-call shape.  One regime is measured the other way: the replace chain of ONE ciphertext at N = 2^14.  Its
// step pass is 2 |Q| workgroups that each walk a whole row twice, while lr_bfv_rotate's launches for a single ciphertext -- both Permutes
// as one launch, the key switch straight into the destination, one Add -- leave nothing for the pass to save but that Add: 1599 us
// against 1573 us for 13 steps at PN14QP438.  From two ciphertexts on the pass wins everywhere.
ChainRoute chain_route(const lr_ckks_plan *pl, int batch, bool accumulate) {
    const int logn = (int)pl->cQ->h.logN;
    if (plan_call_by_call(pl)) return ChainRoute::Composed;
    if (!lr::lds_row_degree(logn) || batch > 65535) return ChainRoute::Composed;
    if (!accumulate && batch == 1 && logn == 14 && !pl->opt.no_pair) return ChainRoute::Composed;
    return ChainRoute::Fused;
}

// the shared checks of the two chain entry points, after their own argument checks: shapes
int check_chain_shapes(const lr_ckks_plan *pl, const lr_poly *c0, const lr_poly *c1, const lr_poly *o0, const lr_poly *o1) {
    LR_TRY(check_call(pl, pl->cQ->h.L() - 1, c0->batch, {c0, c1, o0, o1}));
    return check_permute_degree(pl->cQ);
}

// the chain itself; every argument checked
int chain_core(lr_ckks_plan *pl, const lr_poly *c0, const lr_poly *c1, int n_steps, const u64 *gens, const lr_poly *const *keys, bool accumulate,
               lr_poly *o0, lr_poly *o1) {
    lr_context *cQ = pl->cQ;
    const int batch = c0->batch, L1 = cQ->h.L(), n = (int)cQ->h.N;
    const long long s = poly_words(cQ);
    LR_TRY(begin_pipeline(pl));
    const bool fused = chain_route(pl, batch, accumulate) == ChainRoute::Fused;
    for (Pool *p : {&pl->bfvP, &pl->chainP}) LR_TRY(p->ensure(cQ, (size_t)2 * batch * s));
    for (Pool *p : {&pl->c0, &pl->c2x}) LR_TRY(p->ensure(cQ, (size_t)batch * s));
    u64 *const pair[2] = {pl->bfvP.d, pl->chainP.d};       // each [2][batch][|Q|][N]: back to back, so the key switch's tail takes both halves at once
    auto copy = [&](const Comp &in, const Comp &out) -> int {
        return in.d == out.d ? (int)LR_OK : run_ewise(cQ, LR_COPY, L1, batch, in.d, in.stride, nullptr, 0, out.d, out.stride, nullptr);
    };
    Comp a[2] = {c0, c1};
    const Comp out[2] = {o0, o1};
    int next = 0;      // the pool pair the next key switch accumulates into; the state is never there
    if (out[0].d == a[1].d || out[1].d == a[0].d) {
        // an output over the OTHER component's input: every pass here is local to its own component's row, so the state starts as a copy
        for (int k = 0; k < 2; ++k) {
            const Comp dst(pair[1] + (long long)k * batch * s, s);
            LR_TRY(copy(a[k], dst));
            a[k] = dst;
        }
    }
    if (n_steps == 0) {
        for (int k = 0; k < 2; ++k) LR_TRY(copy(a[k], out[k]));
        return LR_OK;
    }
    if (fused) LR_TRY(run_permute(cQ, false, L1, batch, a[1].d, a[1].stride, pl->c2x.d, s, gens[0]));      // :724 of the first step; the later ones come out of the step pass
    for (int i = 0; i < n_steps; ++i) {
        const bool last = i == n_steps - 1;
        u64 *const p[2] = {pair[next], pair[next] + (long long)batch * s};
        const Comp dst[2] = {last ? out[0] : Comp(p[0], s), last ? out[1] : Comp(p[1], s)};
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
        } else if (accumulate) {
            LR_TRY(bfv_permute_pair(pl, batch, a[0], a[1], gens[i]));                                                          // :723-724
            LR_TRY(bfv_switch_keys_core(pl, batch, pl->c2x.d, s, keys[i], {{p[0], p[1]}, {s, s}}));                            // :729
            LR_TRY(run_ewise(cQ, LR_ADD, L1, batch, pl->c0.d, s, p[0], s, p[0], s, nullptr));                                  // :731
            LR_TRY(run_ewise(cQ, LR_ADD, L1, batch, p[0], s, a[0].d, a[0].stride, dst[0].d, dst[0].stride, nullptr));          // InnerSum :703 / :707
            LR_TRY(run_ewise(cQ, LR_ADD, L1, batch, p[1], s, a[1].d, a[1].stride, dst[1].d, dst[1].stride, nullptr));
        } else {
            // the state is dead once it is permuted: the key switch accumulates straight into the step's destination
            LR_TRY(bfv_rotate_step(pl, batch, a[0], a[1], gens[i], keys[i], dst[0], dst[1]));
        }
        a[0] = dst[0];
        a[1] = dst[1];
        next ^= 1;
    }
    return LR_OK;
}

enum class RelinRoute { Merged, Composed };
// THE route decision of a relinearisation: merged passes of G degrees, unless the plan or its context asks for the
// call-by-call shape.  Measured on one MI355X against the composed route with the same key-switch kernels, in the same run (DESIGN.md
// 6.2, a plan with max_batch 256): the merged route wins wherever G >= 2 -- PN14QP438 degree 5, one ciphertext 148 us against 457 us, 64
// ciphertexts 1621 against 1782; PN13QP218 degree 3, one ciphertext 105 against 182 -- and with G = 1 (the batch fills max_batch: per
// degree the same key switch, then one fold instead of two Adds) the two are within the spread of the repeated medians at every size
// measured (PN14QP438 degree 5 at 256: 6432 against 6397 us, spread 80).  No regime goes to the composed route on speed.
RelinRoute relin_route(const lr_ckks_plan *pl) {
    if (plan_call_by_call(pl)) return RelinRoute::Composed;
    return RelinRoute::Merged;
}

// the relinearisation itself; every argument checked
int relin_core(lr_ckks_plan *pl, const lr_poly *const *ct, int degree, const lr_poly *const *evks, lr_poly *o0, lr_poly *o1) {
    lr_context *cQ = pl->cQ;
    const int batch = ct[0]->batch, L1 = cQ->h.L(), n = (int)cQ->h.N;
    const long long s = poly_words(cQ);
    LR_TRY(begin_pipeline(pl));
    Comp a[2] = {ct[0], ct[1]};           // the running pair
    const Comp out[2] = {o0, o1};
    if (degree == 1) {
        for (int k = 0; k < 2; ++k)
            if (a[k].d != out[k].d) LR_TRY(run_ewise(cQ, LR_COPY, L1, batch, a[k].d, a[k].stride, nullptr, 0, out[k].d, out[k].stride, nullptr));
        return LR_OK;
    }
    if (relin_route(pl) == RelinRoute::Composed) {
        for (int deg = degree; deg > 1; --deg) {
            LR_TRY(bfv_relin_composed_step(pl, batch, ct[deg], evks[deg - 2], a, out));
            a[0] = out[0];
            a[1] = out[1];
        }
        return LR_OK;
    }
    // G groups per pass, the highest degrees first: G * batch <= max_batch, so no pool grows beyond what a call at max_batch needs
    const int G = std::min(degree - 1, std::max(1, pl->max_batch / batch));
    for (int top = degree; top > 1;) {
        const int g = std::min(G, top - 1), members = g * batch;
        LR_TRY(pl->bfvP.ensure(cQ, (size_t)2 * members * s));
        u64 *const p0 = pl->bfvP.d, *const p1 = pl->bfvP.d + (long long)members * s;        // back to back: the tail takes both at once
        Comp cx = ct[top];
        const lr_poly *keys[kBfvRelinFoldTerms];
        for (int i = 0; i < g; ++i) keys[i] = evks[top - i - 2];
        if (g > 1) {
            // the pass's input: ct[top], ct[top - 1], ... as one batch of g * batch members
            LR_TRY(pl->c2x.ensure(cQ, (size_t)members * s));
            MultiCopyLaunch M{};
            for (int i = 0; i < g; ++i) {
                M.src[i] = ct[top - i]->d; M.src_stride[i] = ct[top - i]->stride();
                M.dst[i] = pl->c2x.d + (long long)i * batch * s; M.dst_stride[i] = s;
            }
            M.count = g; M.batch = batch; M.n = n;
            LR_HIP(launch_multicopy(M, L1, cQ->stream));
            cx = Comp(pl->c2x.d, s);
        }
        LR_TRY(bfv_switch_keys_grouped(pl, batch, g, cx.d, cx.stride, keys, {{p0, p1}, {s, s}}));                          // :493, g degrees
        BfvRelinFoldLaunch F;
        for (int k = 0; k < 2; ++k) {
            F.base[k] = a[k].d; F.base_stride[k] = a[k].stride;
            F.out[k] = out[k].d; F.out_stride[k] = out[k].stride;
        }
        F.p[0] = p0; F.p[1] = p1; F.p_stride = s; F.group_stride = (long long)batch * s;
        F.terms = g;
        F.n = n;
        F.lp = cQ->d_lp;
        LR_HIP(launch_bfv_relin_fold(F, L1, batch, cQ->stream));                                                           // :494-495, g degrees
        a[0] = out[0];
        a[1] = out[1];
        top -= g;
    }
    return LR_OK;
}

}  // namespace
}  // namespace lr_host

extern "C" int lr_bfv_switch_keys(lr_ckks_plan *pl, const lr_poly *cx, const lr_poly *evk, lr_poly *p0, lr_poly *p1) {
    return guarded([&]() -> int {
    if (!pl || !cx || !evk || !p0 || !p1) return fail(LR_ERR_ARG, "null argument");
    const int level = pl->cQ->h.L() - 1;
    if (cx == p0 || cx == p1 || p0 == p1) return fail(LR_ERR_ARG, "bfv switch keys: cx, p0 and p1 must be distinct polys");
    LR_TRY(check_cts(pl, level, cx->batch, {cx, p0, p1}));
    LR_TRY(check_batch(pl, cx->batch));
    LR_TRY(begin_pipeline(pl));
    return bfv_switch_keys_core(pl, cx->batch, cx->d, cx->stride(), evk, {{p0->d, p1->d}, {p0->stride(), p1->stride()}});
    });
}

// bfv.evaluator.Relinearize on a degree-2 ciphertext (bfv/evaluator.go:480-501, 512-524): out = (c0 + p0, c1 + p1) with
// (p0, p1) = switchKeys(c2, evakey[0]); all polys over Q in the coefficient domain.  out0 / out1 may be c0 / c1.
extern "C" int lr_bfv_relinearize(lr_ckks_plan *pl, const lr_poly *c0, const lr_poly *c1, const lr_poly *c2, const lr_poly *evk,
                                  lr_poly *out0, lr_poly *out1) {
    return guarded([&]() -> int {
    if (!pl || !c0 || !c1 || !c2 || !evk || !out0 || !out1) return fail(LR_ERR_ARG, "null argument");
    const int level = pl->cQ->h.L() - 1, batch = c2->batch;
    LR_TRY(check_cts(pl, level, batch, {c0, c1, c2, out0, out1}));
    if (out0 == out1 || c2 == out0 || c2 == out1) return fail(LR_ERR_ARG, "bfv relinearize: out0, out1 and c2 must be distinct polys");
    LR_TRY(check_batch(pl, batch));
    LR_TRY(begin_pipeline(pl));
    return bfv_relin_composed_step(pl, batch, c2, evk, {c0, c1}, {out0, out1});
    });
}

// bfv.evaluator.permute (bfv/evaluator.go:711-735), the body of RotateRows (:670-681) and of RotateColumns with the key of that
// rotation (:590-592, and each step of rotateColumnsPow2 :636-662): one bfv_rotate_step into the caller's outputs.
extern "C" int lr_bfv_rotate(lr_ckks_plan *pl, const lr_poly *c0, const lr_poly *c1, uint64_t gen, const lr_poly *rotkey, lr_poly *o0,
                             lr_poly *o1) {
    return guarded([&]() -> int {
    if (!pl || !c0 || !c1 || !rotkey || !o0 || !o1) return fail(LR_ERR_ARG, "null argument");
    lr_context *cQ = pl->cQ;
    const int batch = c0->batch;
    LR_TRY(check_call(pl, cQ->h.L() - 1, batch, {c0, c1, o0, o1}));
    if (o0->d == o1->d) return fail(LR_ERR_ARG, "bfv rotate: the two output polys must be distinct");
    LR_TRY(check_permute_degree(cQ));
    LR_TRY(begin_pipeline(pl));
    for (Pool *p : {&pl->c0, &pl->c2x}) LR_TRY(p->ensure(cQ, (size_t)batch * poly_words(cQ)));
    return bfv_rotate_step(pl, batch, c0, c1, gen, rotkey, o0, o1);
    });
}

// rotateColumnsPow2 (bfv/evaluator.go:637-666) with the caller's elements and keys; InnerSum is its accumulating form
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

// InnerSum (bfv/evaluator.go:691-708): the accumulating chain over the column rotations by 2^i, with the row rotation at the end
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

extern "C" int lr_bfv_relinearize_deg(lr_ckks_plan *pl, const lr_poly *const *ct, int degree, const lr_poly *const *evks, lr_poly *o0,
                                      lr_poly *o1) {
    return guarded([&]() -> int {
    if (!pl || !ct || !o0 || !o1) return fail(LR_ERR_ARG, "null argument");
    if (degree < 1 || degree > 5) return fail(LR_ERR_ARG, "bfv relinearize: the degree must be 1 .. 5");
    for (int k = 0; k <= degree; ++k)
        if (!ct[k]) return fail(LR_ERR_ARG, "null argument");
    if (degree >= 2) {
        if (!evks) return fail(LR_ERR_ARG, "null argument");
        for (int k = 0; k + 2 <= degree; ++k)
            if (!evks[k]) return fail(LR_ERR_ARG, "null argument");
    }
    if (o0 == o1 || o0->d == o1->d) return fail(LR_ERR_ARG, "bfv relinearize: the two output polys must be distinct");
    for (int k = 2; k <= degree; ++k)
        if (ct[k] == o0 || ct[k] == o1 || ct[k]->d == o0->d || ct[k]->d == o1->d)
            return fail(LR_ERR_ARG, "bfv relinearize: an output must not be a component of degree 2 or more");
    if (o0 == ct[1] || o0->d == ct[1]->d || o1 == ct[0] || o1->d == ct[0]->d)
        return fail(LR_ERR_ARG, "bfv relinearize: an output must not be the other component's input");
    const int level = pl->cQ->h.L() - 1, batch = ct[0]->batch;
    LR_TRY(check_batch(pl, batch));
    for (int k = 0; k <= degree; ++k) LR_TRY(check_ct(pl, level, ct[k], batch));
    LR_TRY(check_cts(pl, level, batch, {o0, o1}));
    for (int k = 0; k + 2 <= degree; ++k)
        if (!switching_key_ok(pl, level, evks[k])) return fail(LR_ERR_SHAPE, "evaluation key: need batch >= 2*beta and |Q|+|P| limbs");
    return relin_core(pl, ct, degree, evks, o0, o1);
    });
}
