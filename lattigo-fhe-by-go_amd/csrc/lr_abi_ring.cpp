// lr_abi_ring.cpp -- C ABI: the ring.Context methods -- NTT dispatch (assembly code objects / C++ kernels), the coefficient-wise family,
// Galois automorphisms, SimpleScaler, the RNS rescale -- and the context diagnostics.
#include "lr_host.hpp"

// ------------------------------------------------------------------------------------------
// NTT
// ------------------------------------------------------------------------------------------
namespace lr_host {

// The forward kernels with the subtract-multiply-add epilogue: the dual kernels "m4" (FP64 body below 2^46, integer body -- mode 2 -- for
// the other limbs) where the context runs the dual kernels, the integer kernels "m5" where it runs mode 1 (q <= 2^60: the reference's
// 60-bit rings).  Contexts on the other integer variants (q up to 2^61, or every modulus in [2^46, 2^57)) keep the separate pass.
bool ntt_epilogue_ok(const lr_context *c) {
    const unsigned logn = c->h.logN;
    if (!c->use_asm || logn < 12 || logn > 16 || !ntt_asm_available((int)logn) || c->opt.no_epilogue) return false;
    return c->asm_fwd == 3 || (c->asm_fwd == 1 && !c->opt.no_int_epilogue);
}
// does limb l of the context take the epilogue (otherwise: plain transform + submul_kernel)?
bool ntt_epilogue_limb(const lr_context *c, int l) {
    if (!ntt_epilogue_ok(c)) return false;
    return c->asm_fwd == 1 || c->h.q[l] < kFpLimit || !c->opt.no_int_epilogue;
}
// the epilogue constant cc (plain domain, below q) of limb l in the form that limb's kernel body reads
EpiLimb make_epi_limb(const lr_context *c, int l, u64 cc) {
    const u64 q = c->h.q[l];
    if (c->asm_fwd == 3 && q < kFpLimit) return EpiLimb{(double)cc, (double)cc / (double)q};
    const u64 pair[2] = {cc, shoup_companion(cc, q)};
    EpiLimb e;
    static_assert(sizeof(e) == sizeof(pair), "EpiLimb is 16 bytes");
    std::memcpy(&e, pair, sizeof e);
    return e;
}

// Fork: launches of the calling thread that go to a plan's auxiliary stream instead of the context's (PlanFork, lr_abi_ckks.cpp): two independent
// transforms of a small batch run side by side instead of one after the other.  Only forward transforms are forked (they lease no scratch).
thread_local hipStream_t g_fork_stream = nullptr;

// ---- launch-size policies: each is asked by the route decision (ntt_route) and nowhere else on the transform path
// N = 2^15 transforms as two 2^14 sub-blocks: for launches of at most Options::split15_max_workgroups (128) workgroups -- split, they still fit
// one round on the 256 CUs.  A launch too small to fill the chip with one workgroup per transform (a one-workgroup 2^15 transform takes ~42 us
// whatever surrounds it) gets twice the workgroups at about half the latency on the "h" kernels; the stage over index bit 14 is the streaming
// ntt_top_kernel's (forward: before; inverse: after, with the scaling).
bool ntt_split15(const lr_context *c, long long workgroups) {
    if (c->h.logN != 15 || !c->use_asm || c->opt.timeline || !ntt_asm_available(15)) return false;
    if (c->asm_fwd < 0 || c->asm_inv < 0) return false;
    if (c->opt.split15 >= 0) return c->opt.split15 == 1;
    if (c->opt.persist > 0) return false;          // (LR_NTT_PERSIST asks for the persistent one-workgroup kernels: diagnostics)
    return workgroups <= c->opt.split15_max_workgroups;
}
// N = 2^14: 512 threads per transform put two workgroups on a CU (best throughput); a launch that does not fill the chip anyway takes
// the 1024-thread plan, whose one workgroup is done sooner (PN14QP438, one ciphertext: MulRelin 115 -> 102 us, BFV Mul 136 -> 125 us)
static bool ntt_wide14(const lr_context *c, long long transforms) {
    return c->opt.asm14_1024 || (c->h.logN == 14 && !c->opt.no_wide14_small && transforms <= c->opt.wide14_max_items);
}
// Polys per workgroup of the persistent forward 2^15 kernels (0 = the one-poly kernels, the default): Options::persist, at most the polys of
// a digit group (diagnostics builds)
static int ntt_persist(const lr_context *c, bool inverse, int polys) {
    if (c->h.logN != 15 || inverse) return 0;
    const int p = std::min(c->opt.persist, polys);
    return p >= 2 ? p : 0;
}

// One launch's worth of run_ntt's arguments (the batch is already cut into chunks).
// pretop (forward, N = 2^15 / 2^16 on the assembly kernels): the producer of the input rows has already applied the stage over the top index
// bit (ext_sum_kernel<.., true>, the rescale's streaming pass); the launch goes straight to the plain sub-block kernels, which read their own
// half only.  At N = 2^15 the caller has thereby decided for the split itself.
// lazy (inverse, N = 2^15 / 2^16 on the assembly sub-block kernels): the rows are left as the two halves of every limb before the last
// Gentleman-Sande stage and the scaling -- for a consumer that applies them itself (the top-stage basis extension, ExtLaunch::inv_top)
struct NttRequest {
    bool inverse;
    Rows in, out;
    int mod0, mod_step, count, batch, hole, group;
    const NttEpilogue *epi;
    bool pretop, lazy;
};

// the launch struct of a request: addressing, the direction's tables, and for the dual kernels ("m3" / "m4") the FP64 tables beside them
static NttLaunch ntt_launch_args(const lr_context *c, const NttRequest &q) {
    NttLaunch a{};
    a.in = q.in.base;
    a.out = q.out.base;
    a.in_poly_stride = q.in.stride;
    a.out_poly_stride = q.out.stride;
    a.in_limb0 = q.in.limb0;
    a.in_limb_step = q.in.step;
    a.out_limb0 = q.out.limb0;
    a.out_limb_step = q.out.step;
    a.mod0 = q.mod0;
    a.mod_step = q.mod_step;
    a.n_items = q.count;
    a.batch = q.batch;
    a.hole = q.hole;
    a.group = q.group;
    a.lp = c->d_lp;
    a.tw = q.inverse ? c->d_inv : c->d_fwd;
    a.tw_fin = q.inverse ? c->d_inv_fin : c->d_fwd_fin;
    if ((q.inverse ? c->asm_inv : c->asm_fwd) == 3) {
        a.fp_tw_delta = (const char *)(q.inverse ? c->d_inv_fp : c->d_fwd_fp) - (const char *)a.tw;
        a.fp_fin_delta = (const char *)(q.inverse ? c->d_inv_fin_fp : c->d_fwd_fin_fp) - (const char *)a.tw_fin;
        a.fp_lp = c->d_fp_lp;
    }
    return a;
}
// the next kernel continues in place on the output rows
static void continue_on_output(NttLaunch &a) {
    a.in = a.out;
    a.in_poly_stride = a.out_poly_stride;
    a.in_limb0 = a.out_limb0;
    a.in_limb_step = a.out_limb_step;
}
static void with_epilogue(NttLaunch &a, const NttEpilogue &epi) {
    a.epi_x = epi.x;
    a.epi_x_stride = epi.x_stride;
    a.epi_plus = epi.plus;
    a.epi_plus_stride = epi.plus_stride;
    a.epi_consts = epi.consts;
}

// Which kernels a request takes.  "asm": the context runs the assembly kernels of the request's direction at its degree (variant >= 0);
// "disjoint": no input row is an output row (ntt_rows_disjoint).  An epilogue selects the variant (4 on the dual kernels, 5 on the integer
// ones), never the route's shape; it comes with the forward routes marked (e).
//   N            asm   direction   asked for / launch size                     route
//   any          no    either      --                                          Cxx             the C++ kernels (2^16: their own two passes)
//   <= 2^14      yes   either      --                                          Whole (e)       one kernel per transform (2^14: ntt_wide14 picks the plan)
//   2^15         yes   either      no epilogue, ntt_split15 says no            Whole           (ntt_timeline: Stamped, plain launches of variant 1 / 3)
//   2^15         yes   forward     epilogue without pretop                     Whole (e)       whatever the launch size
//   2^15         yes   forward     pretop                                      Split15Pretop (e)   the 2^14 sub-blocks alone
//   2^15         yes   forward     ntt_split15 says yes                        Split15Top      top pass, then the sub-blocks on the output rows
//   2^15         yes   inverse     lazy                                        Split15InvLazy  the sub-blocks alone
//   2^15         yes   inverse     ntt_split15 says yes (or pretop)            Split15InvTop   the sub-blocks, then the top pass with the scaling
//   2^16         yes   forward     pretop                                      Fwd16Pretop (e) the 2^15 sub-blocks alone
//   2^16         yes   forward     disjoint                                    Fwd16Fused (e)  the top stage inside the sub-blocks' loads
//   2^16         yes   forward     otherwise (no epilogue)                     Fwd16Top        top pass, then the sub-blocks on the output rows
//   2^16         yes   inverse     lazy                                        Inv16Lazy       the sub-blocks alone
//   2^16         yes   inverse     plain launch, not no_invfuse                Inv16PairFlags  the second finisher of a limb's two sub-blocks does the last stage
//   2^16         yes   inverse     otherwise                                   Inv16Top        the sub-blocks, then the top pass with the scaling
// Refused (LR_ERR_ARG): lazy unless inverse, without epilogue, N = 2^15 / 2^16, asm; pretop without epilogue unless N = 2^15 / 2^16, asm (an
// inverse launch ignores it); an epilogue unless forward, plain launch (no digit groups), ntt_epilogue_ok, and at N = 2^16 pretop or disjoint.
struct NttRoute {
    enum Kind { Refused, Cxx, Whole, Stamped, Split15Top, Split15Pretop, Split15InvTop, Split15InvLazy,
                Fwd16Pretop, Fwd16Fused, Fwd16Top, Inv16Lazy, Inv16PairFlags, Inv16Top } kind;
    int variant;             // of the assembly kernels
    bool wide14;             // Whole
    int persist;             // Whole, Stamped
    int code;                // Refused
    const char *why;
};
static NttRoute ntt_route(const lr_context *c, const NttRequest &q) {
    const unsigned logn = c->h.logN;
    const auto refuse = [](int code, const char *why) { return NttRoute{NttRoute::Refused, -1, false, 0, code, why}; };
    if (logn < 1 || logn > 16) return refuse(LR_ERR_UNSUPPORTED, "NTT kernels cover 2 <= N <= 2^16");
    const int own = q.inverse ? c->asm_inv : c->asm_fwd;
    const bool assembly = own >= 0 && c->use_asm && ntt_asm_available((int)logn), sub_blocks = assembly && (logn == 15 || logn == 16);
    const bool disjoint16 = logn == 16 && !q.inverse && !q.pretop && ntt_rows_disjoint(ntt_launch_args(c, q), 16);
    if (q.lazy && !(q.inverse && !q.epi && sub_blocks))
        return refuse(LR_ERR_ARG, "lazy inverse outputs: assembly sub-block kernels of N = 2^15 / 2^16 only");
    if (q.pretop && !q.epi && !sub_blocks)       // (with an epilogue, the epilogue's own conditions decide: ntt_epilogue_ok asks for the assembly kernels)
        return refuse(LR_ERR_ARG, "pre-applied top stage: assembly sub-block kernels of N = 2^15 / 2^16 only");
    if (q.epi && (q.inverse || q.hole > 0 || !ntt_epilogue_ok(c) || (logn == 16 && !q.pretop && !disjoint16)))
        return refuse(LR_ERR_ARG, "NTT epilogue: not available for this launch");
    const auto route = [&](NttRoute::Kind kind) { return NttRoute{kind, q.epi ? (c->asm_fwd == 3 ? 4 : 5) : own, false, 0, LR_OK, nullptr}; };
    const long long transforms = (long long)q.count * q.batch;
    if (logn == 15 && (q.pretop || q.lazy || (!q.epi && ntt_split15(c, transforms)))) {
        if (!q.inverse) return route(q.pretop ? NttRoute::Split15Pretop : NttRoute::Split15Top);
        return route(q.lazy ? NttRoute::Split15InvLazy : NttRoute::Split15InvTop);
    }
    if (logn == 16 && assembly) {
        if (!q.inverse) return route(q.pretop ? NttRoute::Fwd16Pretop : disjoint16 ? NttRoute::Fwd16Fused : NttRoute::Fwd16Top);
        return route(q.lazy ? NttRoute::Inv16Lazy : !c->opt.no_invfuse && q.hole == 0 ? NttRoute::Inv16PairFlags : NttRoute::Inv16Top);
    }
    if (!assembly) return route(NttRoute::Cxx);
    NttRoute r = route(NttRoute::Whole);
    if (q.epi) {
        r.wide14 = ntt_wide14(c, transforms);
        return r;
    }
    r.persist = ntt_persist(c, q.inverse, q.hole > 0 ? q.group : q.batch);
    if (c->opt.timeline && logn == 15 && (own == 1 || own == 3) && q.hole == 0) r.kind = NttRoute::Stamped;   // (the stamped build of the same kernel)
    else r.wide14 = ntt_wide14(c, transforms);
    return r;
}

// diagnostics: the stamps of a Stamped launch land in the context's buffer (lr_context_timeline), which grows to the launch
static int grow_stamps(lr_context *c, size_t words) {
    if (words > c->stamp_words) {
        LR_HIP(hipStreamSynchronize(stream_of(c)));
        if (c->d_stamps) LR_HIP(hipFree(c->d_stamps));
        c->d_stamps = nullptr;
        c->stamp_words = 0;
        LR_HIP(hipMalloc((void **)&c->d_stamps, words * sizeof(u32)));
        c->stamp_words = words;
    }
    c->stamp_used = words;
    return LR_OK;
}

// one request: the route, then its one or two launches
static int run_ntt_launch(lr_context *c, const NttRequest &q) {
    const NttRoute r = ntt_route(c, q);
    if (r.kind == NttRoute::Refused) return fail(r.code, r.why);
    NttLaunch a = ntt_launch_args(c, q);
    if (q.epi) with_epilogue(a, *q.epi);
    // the launcher writes the kernel's name into a local buffer; it reaches the context under its diagnostics mutex on every way out
    struct KernelNote {
        lr_context *c;
        char buf[32];
        ~KernelNote() {
            if (!buf[0]) return;
            std::lock_guard<std::mutex> lock(c->diag_mu);
            std::memcpy(c->last_ntt_kernel, buf, sizeof buf);
        }
    } note{c, ""};
    char *kn = note.buf;
    const hipStream_t s = stream_of(c);
    const int logn = (int)c->h.logN, stagger = c->opt.stagger;
    const bool pad = !c->opt.no_grid_padding;
    switch (r.kind) {
    case NttRoute::Cxx:
        std::snprintf(note.buf, sizeof note.buf, "ntt_%s_kernel<%d>", q.inverse ? "inv" : "fwd", logn);
        LR_HIP(launch_ntt(a, logn, q.inverse, c->ntt_mode, s));
        break;
    case NttRoute::Whole:
        LR_HIP(launch_ntt_asm(a, logn, q.inverse, r.variant, s, r.wide14, kn, false, stagger, r.persist, pad));
        break;
    case NttRoute::Stamped: {
        const size_t words = (size_t)q.batch * (size_t)q.count * 16 * 16;
        LR_TRY(grow_stamps(c, words));
        a.epi_x = reinterpret_cast<const u64 *>(c->d_stamps);
        LR_HIP(launch_ntt_asm(a, logn, q.inverse, r.variant, s, false, kn, true, stagger, r.persist, pad));
        break;
    }
    case NttRoute::Split15Top:
        LR_HIP(launch_ntt_top(a, 0, s, 15));
        continue_on_output(a);
        LR_HIP(launch_ntt_asm16(a, 0, 'h', r.variant, s, kn, stagger, 15));
        break;
    case NttRoute::Split15Pretop:
    case NttRoute::Split15InvLazy:
        LR_HIP(launch_ntt_asm16(a, q.inverse, 'h', r.variant, s, kn, stagger, 15));
        break;
    case NttRoute::Split15InvTop:
        LR_HIP(launch_ntt_asm16(a, 1, 'h', r.variant, s, kn, stagger, 15));
        continue_on_output(a);
        LR_HIP(launch_ntt_top(a, 1, s, 15));
        break;
    case NttRoute::Fwd16Pretop:
        LR_HIP(launch_ntt_asm16(a, 0, 'p', r.variant, s, kn, stagger));
        break;
    case NttRoute::Fwd16Fused:
    case NttRoute::Inv16Lazy:
        LR_HIP(launch_ntt_asm16(a, q.inverse, 's', r.variant, s, kn, stagger));
        break;
    case NttRoute::Fwd16Top:
        LR_HIP(launch_ntt_top(a, 0, s));
        continue_on_output(a);
        LR_HIP(launch_ntt_asm16(a, 0, 'p', r.variant, s, kn, stagger));
        break;
    case NttRoute::Inv16PairFlags: {
        // the wave that finishes second of a limb's two sub-blocks combines both halves (gen_intt.py: fused_last); one u32 flag per wave
        // pair, zeroed here, addressed through NttLaunch::epi_x
        ScratchLease flags;
        const size_t flag_bytes = (size_t)q.batch * (size_t)q.count * 16 * sizeof(u32);
        LR_TRY(flags.take(&c->scratch, (flag_bytes + 7) / 8));
        LR_HIP(hipMemsetAsync(flags.d(), 0, flag_bytes, s));
        a.epi_x = flags.d();
        LR_HIP(launch_ntt_asm16(a, 1, 'f', r.variant, s, kn, stagger));
        break;
    }
    case NttRoute::Inv16Top:
        LR_HIP(launch_ntt_asm16(a, 1, 's', r.variant, s, kn, stagger));
        continue_on_output(a);
        LR_HIP(launch_ntt_top(a, 1, s));
        break;
    case NttRoute::Refused: break;
    }
    return LR_OK;
}

// The assembly kernels of the integer variants put the polynomial on grid.y (limit 65535): longer plain launches are cut into
// chunks along the batch on the same kernel (no silent change of code path).  Grouped launches (key-switch digits) beyond
// the limit are refused: 65536 ciphertexts in one key switch exceed the device memory by orders of magnitude.
int run_ntt(lr_context *c, bool inverse, Rows in, Rows out, int mod0, int mod_step, int count, int batch, int hole,
            int group, const NttEpilogue *epi, bool pretop, bool lazy) {
    if (count <= 0 || batch <= 0) return LR_OK;
    if (hole > 0 && (group <= 0 || batch % group != 0)) return fail(LR_ERR_ARG, "digit groups must divide the batch");
    // N = 2^16: the streaming top-stage kernel carries poly * limbs on grid.y
    const int kChunk = c->h.logN == 16 || (c->h.logN == 15 && c->opt.split15 == 1) ? std::max(1, 65535 / count) : 65535;
    if (hole > 0) {
        if (group > kChunk || batch / group > 65535) return fail(LR_ERR_UNSUPPORTED, "grouped NTT launch: more than 65535 polys per digit group");
        return run_ntt_launch(c, NttRequest{inverse, in, out, mod0, mod_step, count, batch, hole, group, epi, pretop, lazy});
    }
    for (int b0 = 0; b0 < batch; b0 += kChunk) {
        NttRequest q{inverse, in, out, mod0, mod_step, count, std::min(kChunk, batch - b0), 0, 0, epi, pretop, lazy};
        q.in.base = in.base + (long long)b0 * in.stride;
        q.out.base = out.base + (long long)b0 * out.stride;
        NttEpilogue e2;
        if (epi) {
            e2 = *epi;
            e2.x = epi->x + (long long)b0 * epi->x_stride;
            e2.plus = epi->plus + (long long)b0 * epi->plus_stride;
            q.epi = &e2;
        }
        LR_TRY(run_ntt_launch(c, q));
    }
    return LR_OK;
}

int check_pair(const lr_context *c, int level, const lr_poly *in, const lr_poly *out) {
    if (!c || !in || !out) return fail(LR_ERR_ARG, "null argument");
    if (in->N != c->h.N || out->N != c->h.N) return fail(LR_ERR_SHAPE, "ring degree mismatch");
    if (level < 0 || level + 1 > c->h.L()) return fail(LR_ERR_SHAPE, "level exceeds the context's modulus count");
    if (level + 1 > in->limbs || level + 1 > out->limbs) return fail(LR_ERR_SHAPE, "poly has fewer limbs than level+1");
    if (in->batch != out->batch && in->batch != 1) return fail(LR_ERR_SHAPE, "batch mismatch");
    return LR_OK;
}

Rows rows_of(const lr_poly *p, int limb0, int step, bool broadcast_ok, int target_batch) {
    Rows r;
    r.base = p->d;
    r.stride = (broadcast_ok && p->batch == 1 && target_batch > 1) ? 0 : p->stride();
    r.limb0 = limb0;
    r.step = step;
    return r;
}

}  // namespace lr_host

extern "C" int lr_ntt(lr_context *c, int level, const lr_poly *in, lr_poly *out) {
    return guarded([&]() -> int {
    LR_TRY(check_pair(c, level, in, out));
    if (in->batch != out->batch) return fail(LR_ERR_SHAPE, "batch mismatch");
    LR_HIP(hipSetDevice(c->device));
    return run_ntt(c, false, rows_of(in), rows_of(out), 0, 1, level + 1, out->batch);
    });
}

extern "C" int lr_intt(lr_context *c, int level, const lr_poly *in, lr_poly *out) {
    return guarded([&]() -> int {
    LR_TRY(check_pair(c, level, in, out));
    if (in->batch != out->batch) return fail(LR_ERR_SHAPE, "batch mismatch");
    LR_HIP(hipSetDevice(c->device));
    return run_ntt(c, true, rows_of(in), rows_of(out), 0, 1, level + 1, out->batch);
    });
}

static int ntt_limb(lr_context *c, bool inverse, int mod_index, const lr_poly *in, int in_limb, lr_poly *out, int out_limb) {
    if (!c || !in || !out) return fail(LR_ERR_ARG, "null argument");
    if (mod_index < 0 || mod_index >= c->h.L()) return fail(LR_ERR_SHAPE, "modulus index out of range");
    if (in_limb < 0 || in_limb >= in->limbs || out_limb < 0 || out_limb >= out->limbs)
        return fail(LR_ERR_SHAPE, "limb index out of range");
    if (in->batch != out->batch) return fail(LR_ERR_SHAPE, "batch mismatch");
    LR_HIP(hipSetDevice(c->device));
    return run_ntt(c, inverse, rows_of(in, in_limb, 0), rows_of(out, out_limb, 0), mod_index, 0, 1, out->batch);
}

extern "C" int lr_ntt_limb(lr_context *c, int mod_index, const lr_poly *in, int in_limb, lr_poly *out, int out_limb) {
    return guarded([&]() -> int {
    return ntt_limb(c, false, mod_index, in, in_limb, out, out_limb);
    });
}
extern "C" int lr_intt_limb(lr_context *c, int mod_index, const lr_poly *in, int in_limb, lr_poly *out, int out_limb) {
    return guarded([&]() -> int {
    return ntt_limb(c, true, mod_index, in, in_limb, out, out_limb);
    });
}

static int ntt_host(lr_context *c, bool inverse, int level, const uint64_t *const *in_limbs, uint64_t *const *out_limbs) {
    if (!c || !in_limbs || !out_limbs) return fail(LR_ERR_ARG, "null argument");
    if (level < 0 || level + 1 > c->h.L()) return fail(LR_ERR_SHAPE, "level exceeds the context's modulus count");
    lr_poly *tmp = nullptr;
    LR_TRY(lr_poly_alloc(c, level + 1, 1, &tmp));
    int rc = lr_poly_upload(tmp, 0, in_limbs, level + 1);
    if (rc == LR_OK) rc = inverse ? lr_intt(c, level, tmp, tmp) : lr_ntt(c, level, tmp, tmp);
    if (rc == LR_OK) rc = lr_poly_download(tmp, 0, out_limbs, level + 1);
    lr_poly_free(tmp);
    return rc;
}

// the package-level ring.NTT / ring.InvNTT (ring/ntt.go:53,89): one limb under modulus `mod_index` of the context, host slices in
// and out (upload, kernel, download); may be in place
extern "C" int lr_ntt_host_limb(lr_context *c, int mod_index, int inverse, const uint64_t *in, uint64_t *out) {
    return guarded([&]() -> int {
    if (!c || !in || !out) return fail(LR_ERR_ARG, "null argument");
    if (mod_index < 0 || mod_index >= c->h.L()) return fail(LR_ERR_SHAPE, "modulus index out of range");
    lr_poly *tmp = nullptr;
    LR_TRY(lr_poly_alloc(c, 1, 1, &tmp));
    int rc = lr_poly_upload_limb(tmp, 0, 0, in);
    if (rc == LR_OK) rc = ntt_limb(c, inverse != 0, mod_index, tmp, 0, tmp, 0);
    if (rc == LR_OK) rc = lr_poly_download_limb(tmp, 0, 0, out);
    lr_poly_free(tmp);
    return rc;
    });
}

extern "C" int lr_ntt_host(lr_context *c, int level, const uint64_t *const *in_limbs, uint64_t *const *out_limbs) {
    return guarded([&]() -> int {
    return ntt_host(c, false, level, in_limbs, out_limbs);
    });
}
extern "C" int lr_intt_host(lr_context *c, int level, const uint64_t *const *in_limbs, uint64_t *const *out_limbs) {
    return guarded([&]() -> int {
    return ntt_host(c, true, level, in_limbs, out_limbs);
    });
}

// ------------------------------------------------------------------------------------------
// coefficient-wise
// ------------------------------------------------------------------------------------------
namespace lr_host {

bool op_reads_b(int op) {
    return op == LR_ADD || op == LR_ADD_NOMOD || op == LR_SUB || op == LR_SUB_NOMOD ||
           (op >= LR_MUL_COEFFS && op <= LR_MUL_MONT_CONSTANT);
}

// raw form used by the pipelines: pointers are already offset to limb 0 of the operands
int run_ewise(lr_context *c, int op, int limbs, int batch, const u64 *a, long long a_stride, const u64 *b,
              long long b_stride, u64 *out, long long out_stride, const LimbScalars *sc, int lp_offset) {
    EwiseLaunch L;
    L.a = a;
    L.b = b;
    L.out = out;
    L.a_stride = a_stride;
    L.b_stride = b_stride;
    L.out_stride = out_stride;
    L.n = (int)c->h.N;
    L.lp = c->d_lp + lp_offset;
    L.has_scalars = sc ? 1 : 0;
    if (sc) L.scalars = *sc;
    LR_HIP(launch_ewise(op, L, limbs, batch, c->stream));
    return LR_OK;
}

}  // namespace lr_host

extern "C" int lr_ewise(lr_context *c, int op, int level, const lr_poly *a, const lr_poly *b, lr_poly *out,
                        const uint64_t *scalars) {
    return guarded([&]() -> int {
    if (!c || !a || !out) return fail(LR_ERR_ARG, "null argument");
    if (op < 0 || op >= LR_EWISE_OP_COUNT) return fail(LR_ERR_ARG, "unknown coefficient-wise op");
    LR_TRY(check_pair(c, level, a, out));
    const bool needs_b = op_reads_b(op);
    if (needs_b) {
        if (!b) return fail(LR_ERR_ARG, "this op needs a second operand");
        LR_TRY(check_pair(c, level, b, out));
    }
    if (c->h.N < 2) return fail(LR_ERR_UNSUPPORTED, "N must be at least 2");
    LR_HIP(hipSetDevice(c->device));
    LimbScalars sc;
    const LimbScalars *scp = nullptr;
    const int limbs = level + 1;
    if (op == LR_MUL_SCALAR || op == LR_MUL_SCALAR_LIMBS || op == LR_ADD_SCALAR_LIMBS || op == LR_SUB_SCALAR_LIMBS ||
        op == LR_MUL_BY_POW2) {
        if (!scalars) return fail(LR_ERR_ARG, "this op needs scalars");
        for (int i = 0; i < limbs; ++i) {
            const u64 q = c->h.q[i];
            const BarrettConst bc = c->h.bred[i];
            switch (op) {
            case LR_MUL_SCALAR: sc.v[i] = mform(bred_add(scalars[0], q, bc.hi), q, bc.hi, bc.lo); break;      // ring.go:516
            case LR_MUL_SCALAR_LIMBS: sc.v[i] = mform(bred_add(scalars[i], q, bc.hi), q, bc.hi, bc.lo); break; // ring.go:547
            case LR_MUL_BY_POW2: sc.v[i] = scalars[0]; break;
            default: sc.v[i] = scalars[i]; break;
            }
        }
        scp = &sc;
    }
    const int batch = out->batch;
    const long long as = (a->batch == 1 && batch > 1) ? 0 : a->stride();
    const long long bs = (b && b->batch == 1 && batch > 1) ? 0 : (b ? b->stride() : 0);
    if (op == LR_MUL_BY_POW2 && a->d == out->d) {
        // MulByPow2 in place: the reference first overwrites p2 with MForm(p1), ring/ring.go:630
        LR_TRY(run_ewise(c, LR_MFORM, limbs, batch, a->d, as, nullptr, 0, out->d, out->stride(), nullptr));
    }
    return run_ewise(c, op, limbs, batch, a->d, as, needs_b ? b->d : nullptr, bs, out->d, out->stride(), scp);
    });
}

// ------------------------------------------------------------------------------------------
// half-vector scalar operations (the constant-by-ciphertext methods of ckks.Evaluator)
// ------------------------------------------------------------------------------------------
extern "C" int lr_half_scalar_op(lr_context *c, int op, int level, const lr_poly *in, const uint64_t *lo, const uint64_t *hi, lr_poly *out) {
    return guarded([&]() -> int {
    LR_TRY(check_pair(c, level, in, out));
    if (in->batch != out->batch) return fail(LR_ERR_SHAPE, "batch mismatch");
    if (!lo || !hi) return fail(LR_ERR_ARG, "null scalar array");
    if (op < 0 || op > 2) return fail(LR_ERR_ARG, "half-vector scalar op: 0 = add, 1 = multiply, 2 = multiply and add");
    if (c->h.N < 4) return fail(LR_ERR_UNSUPPORTED, "half-vector scalar op: ring degree below 4");
    LR_HIP(hipSetDevice(c->device));
    HalfScalarLaunch L;
    L.in = in->d;
    L.out = out->d;
    L.in_stride = in->stride();
    L.out_stride = out->stride();
    L.n = (int)c->h.N;
    L.op = op;
    L.lp = c->d_lp;
    std::memset(&L.lo, 0, sizeof(L.lo));
    std::memset(&L.hi, 0, sizeof(L.hi));
    for (int i = 0; i <= level; ++i) {
        L.lo.v[i] = lo[i];
        L.hi.v[i] = hi[i];
    }
    LR_HIP(launch_half_scalar(L, level + 1, out->batch, c->stream));
    return LR_OK;
    });
}

// ------------------------------------------------------------------------------------------
// Galois automorphisms (ring/ring_galois.go)
// ------------------------------------------------------------------------------------------
// the launch of an automorphism or a monomial product: only gen mod 2N matters in either domain (indices are taken mod 2N resp. mod N
// with the sign from bit logN; MultByMonomial reduces its degree the same way, ring/ring.go:667)
static GaloisLaunch galois_launch(const lr_context *c, const u64 *in, long long in_stride, lr_poly *out, u64 gen, bool ntt_domain) {
    GaloisLaunch L;
    L.in = in;
    L.out = out->d;
    L.in_stride = in_stride;
    L.out_stride = out->stride();
    L.n = (int)c->h.N;
    L.logn = (int)c->h.logN;
    L.ntt_domain = ntt_domain ? 1 : 0;
    L.gen = gen & ((c->h.N << 1) - 1);
    L.lp = c->d_lp;
    return L;
}
// an operation that may not read what it writes, called in place: the input goes through a temporary (as the reference's tmpx,
// ring/ring.go:682-693); *src is the rows to read
static int unaliased_input(lr_context *c, const lr_poly *in, const lr_poly *out, ScratchLease *tmp, const u64 **src) {
    *src = in->d;
    if (in->d != out->d) return LR_OK;
    const size_t words = (size_t)out->batch * (size_t)in->stride();
    LR_TRY(tmp->take(&c->scratch, words));
    LR_HIP(hipMemcpyAsync(tmp->d(), in->d, words * sizeof(u64), hipMemcpyDeviceToDevice, c->stream));
    *src = tmp->d();
    return LR_OK;
}
// Shift's and Rotate's n as Go evaluates n & ((1 << N) - 1): the mask is all ones for N >= 64 and 2^N - 1 below
static u64 mask_shift_count(u64 n, u64 N) { return N >= 64 ? n : (n & (((u64)1 << N) - 1)); }

static int permute_common(lr_context *c, int level, const lr_poly *in, u64 gen, lr_poly *out, bool ntt_domain) {
    LR_TRY(check_pair(c, level, in, out));
    if (in->batch != out->batch) return fail(LR_ERR_SHAPE, "batch mismatch");
    if (in->d == out->d) return fail(LR_ERR_ARG, "Permute is not in place (ring/ring_galois.go:54)");
    if (c->h.N < 2 || c->h.logN > 31) return fail(LR_ERR_UNSUPPORTED, "ring degree");
    LR_HIP(hipSetDevice(c->device));
    LR_HIP(launch_permute(galois_launch(c, in->d, in->stride(), out, gen, ntt_domain), level + 1, out->batch, c->stream));
    return LR_OK;
}

extern "C" int lr_permute_ntt(lr_context *c, int level, const lr_poly *in, uint64_t gen, lr_poly *out) {
    return guarded([&]() -> int {
    if (!c || !in || !out) return fail(LR_ERR_ARG, "null argument");
    return permute_common(c, level, in, gen, out, true);
    });
}

extern "C" int lr_permute(lr_context *c, const lr_poly *in, uint64_t gen, lr_poly *out) {
    return guarded([&]() -> int {
    if (!c || !in || !out) return fail(LR_ERR_ARG, "null argument");
    return permute_common(c, c->h.L() - 1, in, gen, out, false);
    });
}

extern "C" int lr_mult_by_monomial(lr_context *c, const lr_poly *in, uint64_t monomial_deg, lr_poly *out) {
    return guarded([&]() -> int {
    if (!c || !in || !out) return fail(LR_ERR_ARG, "null argument");
    const int level = c->h.L() - 1;
    LR_TRY(check_pair(c, level, in, out));
    if (in->batch != out->batch) return fail(LR_ERR_SHAPE, "batch mismatch");
    LR_HIP(hipSetDevice(c->device));
    ScratchLease tmp;
    const u64 *src = nullptr;
    LR_TRY(unaliased_input(c, in, out, &tmp, &src));
    LR_HIP(launch_monomial(galois_launch(c, src, in->stride(), out, monomial_deg, false), level + 1, out->batch, c->stream));
    return LR_OK;
    });
}

// Context.Shift (ring/ring.go:575-580): p2 = p1 rotated left by n coefficient positions, every limb.  The reference masks n with
// (1 << N) - 1, which in Go is all ones for N >= 64 and 2^N - 1 below, and slices p1.Coeffs[i][n:]: n > N panics (here: LR_ERR_ARG).
extern "C" int lr_shift(lr_context *c, const lr_poly *in, uint64_t n, lr_poly *out) {
    return guarded([&]() -> int {
    if (!c || !in || !out) return fail(LR_ERR_ARG, "null argument");
    const int level = c->h.L() - 1;
    LR_TRY(check_pair(c, level, in, out));
    if (in->batch != out->batch) return fail(LR_ERR_SHAPE, "batch mismatch");
    const u64 N = c->h.N;
    const u64 m = mask_shift_count(n, N);
    if (m > N) return fail(LR_ERR_ARG, "Shift: n exceeds the ring degree (the reference's slice expression panics)");
    LR_HIP(hipSetDevice(c->device));
    ScratchLease tmp;
    const u64 *src = nullptr;
    LR_TRY(unaliased_input(c, in, out, &tmp, &src));
    const size_t pitch = (size_t)N * sizeof(u64), rows = (size_t)(level + 1);
    for (int b = 0; b < out->batch; ++b) {
        const u64 *s = src + (long long)b * in->stride();
        u64 *d = out->d + (long long)b * out->stride();
        if (m < N) LR_HIP(hipMemcpy2DAsync(d, pitch, s + m, pitch, (size_t)(N - m) * sizeof(u64), rows, hipMemcpyDeviceToDevice, c->stream));
        if (m > 0) LR_HIP(hipMemcpy2DAsync(d + (N - m), pitch, s, pitch, (size_t)m * sizeof(u64), rows, hipMemcpyDeviceToDevice, c->stream));
    }
    return LR_OK;
    });
}

// Context.Rotate (ring/ring.go:775-800): coefficient j of every limb is multiplied by omega^(n j), omega = psi^2, for j = 1 .. N-1;
// coefficient 0 is left as it is.  The reference writes the result into p1 whatever p2 is (`p1tmp, p2tmp := p1.Coeffs[i], p1.Coeffs[i]`,
// :791), so this entry point takes one poly.  n is masked like Shift's.  The factors gal_j = MForm(omega^(n j)) are canonical residues and
// MRed(x, gal_j) is the canonical x * omega^(n j): the table is built on the host per call (the reference's only caller is its test
// suite, ring_test.go:435) and applied by the Montgomery product kernel.
extern "C" int lr_rotate(lr_context *c, lr_poly *p1, uint64_t n) {
    return guarded([&]() -> int {
    if (!c || !p1) return fail(LR_ERR_ARG, "null argument");
    const int level = c->h.L() - 1;
    LR_TRY(check_pair(c, level, p1, p1));
    const u64 N = c->h.N;
    if (N < 2) return fail(LR_ERR_UNSUPPORTED, "N must be at least 2");
    const u64 m = mask_shift_count(n, N);
    LR_HIP(hipSetDevice(c->device));
    const int L = level + 1;
    std::vector<u64> gal((size_t)L * N);
    for (int i = 0; i < L; ++i) {
        const u64 q = c->h.q[i], qinv = c->h.mred[i];
        const BarrettConst bc = c->h.bred[i];
        const u64 omega = mred(c->h.psi_mont[i], c->h.psi_mont[i], q, qinv);              // psi^2 in Montgomery form (:785)
        // root = omega^m in Montgomery form (:787): square and multiply on Montgomery residues
        u64 root = mform(1, q, bc.hi, bc.lo), base = omega;
        for (u64 e = m; e > 0; e >>= 1) {
            if (e & 1) root = mred(root, base, q, qinv);
            base = mred(base, base, q, qinv);
        }
        u64 g = mform(1, q, bc.hi, bc.lo);                                               // :789
        gal[(size_t)i * N] = g;
        for (u64 j = 1; j < N; ++j) {
            g = mred(g, root, q, qinv);                                                  // :795
            gal[(size_t)i * N + j] = g;
        }
    }
    ScratchLease table, heads;
    const size_t rows = (size_t)p1->batch * (size_t)L;
    LR_TRY(table.take(&c->scratch, gal.size()));
    LR_TRY(heads.take(&c->scratch, rows));
    // the multiply below is not ordered against a host buffer that dies with this call: finish the upload first
    LR_HIP(hipMemcpyAsync(table.d(), gal.data(), gal.size() * sizeof(u64), hipMemcpyHostToDevice, c->stream));
    LR_HIP(hipStreamSynchronize(c->stream));
    const size_t pitch = (size_t)N * sizeof(u64);
    // coefficient 0 of every row is not touched by the reference (the loop starts at j = 1): keep it aside, put it back afterwards
    for (int b = 0; b < p1->batch; ++b)
        LR_HIP(hipMemcpy2DAsync(heads.d() + (size_t)b * L, sizeof(u64), p1->d + (long long)b * p1->stride(), pitch, sizeof(u64), (size_t)L,
                                hipMemcpyDeviceToDevice, c->stream));
    LR_TRY(run_ewise(c, LR_MUL_MONT, L, p1->batch, p1->d, p1->stride(), table.d(), 0, p1->d, p1->stride(), nullptr));
    for (int b = 0; b < p1->batch; ++b)
        LR_HIP(hipMemcpy2DAsync(p1->d + (long long)b * p1->stride(), pitch, heads.d() + (size_t)b * L, sizeof(u64), sizeof(u64), (size_t)L,
                                hipMemcpyDeviceToDevice, c->stream));
    return LR_OK;
    });
}

extern "C" int lr_permute_ntt_index(uint64_t gen, uint64_t power, uint64_t N, uint64_t *index) {
    return guarded([&]() -> int {
    if (!index) return fail(LR_ERR_ARG, "null argument");
    if (N == 0 || (N & (N - 1)) != 0) return fail(LR_ERR_INVALID_DEGREE, "invalid ring degree (must be a power of 2)");
    const u64 gen_pow = mod_exp(gen, power, 2 * N);
    unsigned logn = 0;
    while ((1ull << logn) < N) ++logn;
    const u64 mask = (N << 1) - 1;
    for (u64 i = 0; i < N; ++i) {
        const u64 t1 = 2 * bit_reverse(i, logn) + 1;
        const u64 t2 = ((gen_pow * t1 & mask) - 1) >> 1;
        index[i] = bit_reverse(t2, logn);
    }
    return LR_OK;
    });
}

// ------------------------------------------------------------------------------------------
// SimpleScaler (ring/ring_scaling.go:166-300)
// ------------------------------------------------------------------------------------------
extern "C" int lr_simple_scaler_create(lr_context *c, uint64_t t, lr_simple_scaler **out) {
    return guarded([&]() -> int {
    if (!out) return fail(LR_ERR_ARG, "out is null");
    *out = nullptr;
    if (!c) return fail(LR_ERR_ARG, "null context");
    std::unique_ptr<lr_simple_scaler> s(new (std::nothrow) lr_simple_scaler);
    if (!s) return fail(LR_ERR_ARG, "out of host memory");
    if (!build_simple_scaler(t, c->h.q, s->h)) return fail(LR_ERR_ARG, "t must be non-zero (BRedParams divides by it, ring/modular_reduction.go:97)");
    s->device = c->device;
    s->ctx = c;
    LR_HIP(hipSetDevice(c->device));
    std::vector<double> ti(2 * s->h.ti.size());
    for (size_t i = 0; i < s->h.ti.size(); ++i) {
        ti[2 * i] = s->h.ti[i].hi;
        ti[2 * i + 1] = s->h.ti[i].lo;
    }
    LR_TRY(to_device(&s->d_wi, s->h.wi.data(), s->h.wi.size()));
    LR_TRY(to_device(&s->d_ti, ti.data(), ti.size()));
    *out = s.release();
    return LR_OK;
    });
}

extern "C" int lr_simple_scaler_destroy(lr_simple_scaler *s) {
    return guarded([&]() -> int {
    if (!s) return LR_OK;
    (void)hipSetDevice(s->device);
    (void)hipDeviceSynchronize();   // the handle's work may be on its contexts' caller-supplied stream
    delete s;
    return LR_OK;
    });
}

extern "C" int lr_simple_scaler_tables(const lr_simple_scaler *s, uint64_t *wi, double *ti, int count) {
    return guarded([&]() -> int {
    if (!s || !wi || !ti) return fail(LR_ERR_ARG, "null argument");
    if (count != (int)s->h.wi.size()) return fail(LR_ERR_SHAPE, "table size mismatch");
    for (int i = 0; i < count; ++i) {
        wi[i] = s->h.wi[i];
        ti[2 * i] = s->h.ti[i].hi;
        ti[2 * i + 1] = s->h.ti[i].lo;
    }
    return LR_OK;
    });
}

extern "C" int lr_simple_scale(lr_simple_scaler *s, const lr_poly *p1, lr_poly *p2) {
    return guarded([&]() -> int {
    if (!s || !p1 || !p2) return fail(LR_ERR_ARG, "null argument");
    lr_context *c = s->ctx;
    if (p1->N != c->h.N || p2->N != c->h.N) return fail(LR_ERR_SHAPE, "ring degree mismatch");
    if (p1->limbs < c->h.L()) return fail(LR_ERR_SHAPE, "p1 must hold every modulus of the scaler's context (index out of range in the reference)");
    if (p1->device != c->device || p2->device != c->device) return fail(LR_ERR_ARG, "poly lives on another device");
    if (p1->batch != p2->batch) return fail(LR_ERR_SHAPE, "batch mismatch");
    LR_HIP(hipSetDevice(c->device));
    ScaleLaunch L;
    L.in = p1->d;
    L.out = p2->d;
    L.in_stride = p1->stride();
    L.out_stride = p2->stride();
    L.wi = s->d_wi;
    L.ti = s->d_ti;
    L.t = s->h.t;
    L.add_param = s->h.add_param;
    L.mul_param = s->h.mul_param;
    L.pow2 = s->h.pow2 ? 1 : 0;
    L.limbs_in = c->h.L();
    L.limbs_out = p2->limbs;
    L.n = (int)c->h.N;
    LR_HIP(launch_simple_scale(L, p1->batch, c->stream));
    return LR_OK;
    });
}

// ------------------------------------------------------------------------------------------
// RNS rescale (ring/ring_scaling.go:9-164)
// ------------------------------------------------------------------------------------------
namespace lr_host {

int check_rescale(lr_context *c, lr_poly *p0) {
    if (!c || !p0) return fail(LR_ERR_ARG, "null argument");
    if (p0->N != c->h.N) return fail(LR_ERR_SHAPE, "ring degree mismatch");
    if (p0->limbs < 2) return fail(LR_ERR_SHAPE, "cannot divide by the last modulus of a 1-limb polynomial");
    if (p0->limbs > c->h.L()) return fail(LR_ERR_SHAPE, "poly has more limbs than the context has moduli");
    return LR_OK;
}

// pHalf = (p_j - 1) / 2 of the last modulus p_j = q[level], and pHalfNegQi[i] = q_i - (pHalf mod q_i) for the limbs below it (:83-89 / :125-129)
static u64 rescale_phalf(const lr_context *c, int level) { return (c->h.q[level] - 1) >> 1; }
static LimbScalars phalf_neg_qi(const lr_context *c, int level) {
    LimbScalars s{};
    for (int i = 0; i < level; ++i) s.v[i] = c->h.q[i] - bred_add(rescale_phalf(c, level), c->h.q[i], c->h.bred[i].hi);
    return s;
}
// the centring: pHalf is added to the last limb, in place (:87-89)
static int add_phalf_to_last(lr_context *c, lr_poly *p0) {
    const int level = p0->limbs - 1;
    RowAddLaunch L;
    L.in = L.out = p0->d + (long long)level * (long long)c->h.N;
    L.in_stride = L.out_stride = p0->stride();
    L.n = (int)c->h.N;
    L.q = c->h.q[level];
    L.adds = LimbScalars{};
    L.adds.v[0] = rescale_phalf(c, level);
    LR_HIP(launch_rowadd(L, 1, p0->batch, c->stream));
    return LR_OK;
}

// round == true adds the pHalf centring
int rescale_coeff_domain(lr_context *c, lr_poly *p0, bool round) {
    const int level = p0->limbs - 1, batch = p0->batch;
    const u64 *last = p0->d + (long long)level * (long long)c->h.N;
    if (round) LR_TRY(add_phalf_to_last(c, p0));
    const LimbScalars add = round ? phalf_neg_qi(c, level) : LimbScalars{};
    LR_TRY(run_submul(c, level, batch, p0->d, p0->stride(), last, p0->stride(), 0, p0->d, p0->stride(),
                      c->d_rescale + (size_t)(level - 1) * c->h.L(), true, &add));
    p0->limbs = level;
    return LR_OK;
}

// The rounding variant transforms (t + pHalfNegQi[i]) under modulus i, t = the centred last limb (:101-105).  The transform is
// linear and the addend is the same in every coefficient: NTT_i(t + a_i * ones) = NTT_i(t) + a_i * NTT_i(ones), so the
// polynomial is transformed as it is (one source row for all limbs, like the floor variant) and the constant vector joins
// the subtract-multiply as its `plus` operand, already multiplied by -rescaleParams[i]: the same canonical residue without the
// pass that writes `level` shifted copies of the row.  The table depends on the level only and is built once.
int rescale_round_table(lr_context *c, int level, const lr_context::RoundTable **out) {
    std::lock_guard<std::mutex> lock(c->rescale_mu);
    auto it = c->rescale_round.find(level);
    if (it != c->rescale_round.end()) {
        *out = &it->second;
        return LR_OK;
    }
    // built into locals; the cache only ever holds complete tables (a failure below leaves no entry behind)
    const int n = (int)c->h.N;
    const long long words = (long long)level * n;
    struct Guard {
        u64 *table = nullptr, *zeros = nullptr;
        EpiLimb *epi = nullptr;
        ~Guard() {
            if (table) (void)hipFree(table);
            if (zeros) (void)hipFree(zeros);
            if (epi) (void)hipFree(epi);
        }
    } g;
    ScratchLease tmpbuf;
    LR_TRY(tmpbuf.take(&c->scratch, (size_t)words));
    LR_HIP(hipMalloc((void **)&g.table, (size_t)words * sizeof(u64)));
    LR_HIP(hipMemsetAsync(g.table, 0, (size_t)words * sizeof(u64), c->stream));
    // the flooring division (DivFloorByLastModulusNTT) takes the same epilogue with nothing to add: rows of zeros in the same layout
    LR_HIP(hipMalloc((void **)&g.zeros, (size_t)words * sizeof(u64)));
    LR_HIP(hipMemsetAsync(g.zeros, 0, (size_t)words * sizeof(u64), c->stream));
    RowAddLaunch M;
    M.in = g.table;                     // a row of zeros
    M.in_stride = 0;
    M.out = tmpbuf.d();
    M.out_stride = words;
    M.n = n;
    M.q = 0;
    M.adds = phalf_neg_qi(c, level);
    LR_HIP(launch_rowadd(M, level, 1, c->stream));
    Rows tmp{tmpbuf.d(), words, 0, 1};
    LR_TRY(run_ntt(c, false, tmp, tmp, 0, 1, level, 1));
    // table = MRed(0 + (q - NTT(a_i * ones)), rescaleParams[i])
    LR_TRY(run_submul(c, level, 1, g.table, words, tmpbuf.d(), words, (long long)n, g.table, words,
                      c->d_rescale + (size_t)(level - 1) * c->h.L(), false, nullptr));
    {
        std::vector<EpiLimb> ec(c->h.L());
        for (int i = 0; i < level; ++i) {
            const u64 q = c->h.q[i], cc = inv_mform(c->h.rescale[(size_t)(level - 1) * c->h.L() + i], q, c->h.mred[i]);
            ec[i] = make_epi_limb(c, i, cc);
        }
        LR_TRY(to_device(&g.epi, ec.data(), ec.size()));
    }
    *out = &(c->rescale_round[level] = lr_context::RoundTable{g.table, g.epi, g.zeros});
    g.table = nullptr;
    g.zeros = nullptr;
    g.epi = nullptr;
    return LR_OK;
}

// What one division in the NTT domain does, decided before its first launch.
//   tables     the level's tables (rescale_round_table), unless rescale_unfused; the flooring division needs them for the epilogue only
//   epilogue   (x - NTT_i(t)) * rescaleParams[i] + addend inside the forward transforms' copy-out, for every run of limbs that takes it
//              (epilogue_run_end); the addend is the rounding's table or, flooring, the rows of zeros.  Otherwise the transforms go to
//              scratch rows and one submul follows
//   plus       the rounding's addend outside the epilogue: the table, or nothing (flooring; unfused rounding shifts the row first instead)
//   fuse_mid   N = 2^15, a small launch whose every target limb takes the epilogue: the last limb's inverse sub-blocks stay lazy and ONE
//              streaming kernel does what lies between them and the targets' forward sub-blocks (last inverse stage + scaling, + pHalf,
//              forward top stage)
struct RescalePlan {
    const lr_context::RoundTable *tables = nullptr;
    bool epilogue = false, fuse_mid = false;
    const u64 *plus = nullptr, *epi_plus = nullptr;
};
static int rescale_plan(lr_context *c, int level, int batch, bool round, RescalePlan *out) {
    RescalePlan p;
    if (!c->opt.rescale_unfused && (round || ntt_epilogue_ok(c))) LR_TRY(rescale_round_table(c, level, &p.tables));
    p.epilogue = p.tables && ntt_epilogue_ok(c);
    if (p.tables) {
        p.plus = round ? p.tables->plus : nullptr;
        p.epi_plus = round ? p.tables->plus : p.tables->zeros;
    }
    p.fuse_mid = round && p.epilogue && c->h.logN == 15 && !c->opt.no_invtop && c->asm_inv >= 0 && ntt_split15(c, (long long)level * batch);
    for (int l = 0; l < level && p.fuse_mid; ++l) p.fuse_mid = ntt_epilogue_limb(c, l);
    *out = p;
    return LR_OK;
}

// the forward transforms of one run of limbs [l0, l1) that takes the epilogue: the last limb's row under each of their moduli, into p0's rows
static int rescale_epilogue_run(lr_context *c, lr_poly *p0, const RescalePlan &plan, u64 *scratch, int l0, int l1) {
    const int level = p0->limbs - 1, batch = p0->batch;
    const long long tmp_stride = (long long)level * (long long)c->h.N;
    const NttEpilogue ep{p0->d, p0->stride(), plan.epi_plus, 0, plan.tables->epi};
    const Rows last{p0->d, p0->stride(), level, 0}, dst{p0->d, p0->stride(), l0, 1};
    if (!ntt_split15(c, (long long)(l1 - l0) * batch)) return run_ntt(c, false, last, dst, l0, 1, l1 - l0, batch, 0, 0, &ep);
    // N = 2^15, a small launch: the transforms with the epilogue on two workgroups each (2^14 sub-blocks).  Every target
    // limb has its own top-stage twiddle, so the stage over bit 14 goes to the scratch rows first (the streaming kernel,
    // the last limb's row broadcast to one row per target limb); the sub-blocks read those and write p0's rows.
    const Rows src{scratch, tmp_stride, l0, 1};
    NttLaunch t = ntt_launch_args(c, NttRequest{false, last, src, l0, 1, l1 - l0, batch, 0, 0, nullptr, false, false});
    t.tw_fin = nullptr;                 // (the streaming kernels read lp and tw alone: their argument block stays as it has been)
    t.fp_tw_delta = t.fp_fin_delta = 0;
    t.fp_lp = nullptr;
    if (plan.fuse_mid) LR_HIP(launch_rescale_mid(t, c->d_inv, level, rescale_phalf(c, level), 15, stream_of(c)));
    else LR_HIP(launch_ntt_top(t, 0, stream_of(c), 15));
    return run_ntt(c, false, src, dst, l0, 1, l1 - l0, batch, 0, 0, &ep, true);
}

int rescale_ntt_domain(lr_context *c, lr_poly *p0, bool round) {
    const int level = p0->limbs - 1, batch = p0->batch;
    const long long n = (long long)c->h.N, tmp_stride = level * n;
    RescalePlan plan;
    LR_TRY(rescale_plan(c, level, batch, round, &plan));
    ScratchLease scratch;
    LR_TRY(scratch.take(&c->scratch, (size_t)batch * tmp_stride));
    const Rows last{p0->d, p0->stride(), level, 0}, tmp{scratch.d(), tmp_stride, 0, 1};
    const u64 *const consts = c->d_rescale + (size_t)(level - 1) * c->h.L();
    // the last limb back to the coefficient domain (:15 / :80), centred (:87-89) unless the streaming kernel between the sub-blocks does both
    LR_TRY(run_ntt(c, true, last, last, level, 0, 1, batch, 0, 0, nullptr, false, plan.fuse_mid));
    if (round && !plan.fuse_mid) LR_TRY(add_phalf_to_last(c, p0));
    if (plan.epilogue) {
        for (int l0 = 0, l1; l0 < level; l0 = l1) {
            bool takes;
            l1 = epilogue_run_end(c, l0, level, &takes);
            if (takes) {
                LR_TRY(rescale_epilogue_run(c, p0, plan, scratch.d(), l0, l1));
                continue;
            }
            LR_TRY(run_ntt(c, false, last, Rows{scratch.d(), tmp_stride, l0, 1}, l0, 1, l1 - l0, batch));
            LR_TRY(run_submul(c, l1 - l0, batch, p0->d + l0 * n, p0->stride(), scratch.d() + l0 * n, tmp_stride, n, p0->d + l0 * n, p0->stride(),
                              consts + l0, false, nullptr, plan.plus ? plan.plus + l0 * n : nullptr, 0, nullptr, l0));
        }
        p0->limbs = level;
        return LR_OK;
    }
    // NTT_i(t) for every limb below the last (:19), then ONE submul; the rounding's shift by pHalfNegQi[i] rides in `plus`, or -- unfused --
    // goes into `level` shifted copies of the row before the transforms (:101-105)
    if (round && !plan.plus) {
        RowAddLaunch M;
        M.in = p0->d + level * n;
        M.in_stride = p0->stride();
        M.out = scratch.d();
        M.out_stride = tmp_stride;
        M.n = (int)n;
        M.q = 0;
        M.adds = phalf_neg_qi(c, level);
        LR_HIP(launch_rowadd(M, level, batch, c->stream));
    }
    LR_TRY(run_ntt(c, false, round && !plan.plus ? tmp : last, tmp, 0, 1, level, batch));
    LR_TRY(run_submul(c, level, batch, p0->d, p0->stride(), scratch.d(), tmp_stride, n, p0->d, p0->stride(), consts, false, nullptr, plan.plus, 0));
    p0->limbs = level;
    return LR_OK;
}

}  // namespace lr_host

// the four single divisions: DivFloor / DivRound ByLastModulus (NTT)
static int rescale_one(lr_context *c, lr_poly *p0, bool ntt_domain, bool round) {
    LR_TRY(check_rescale(c, p0));
    LR_HIP(hipSetDevice(c->device));
    return ntt_domain ? rescale_ntt_domain(c, p0, round) : rescale_coeff_domain(c, p0, round);
}
extern "C" int lr_div_floor_by_last_modulus_ntt(lr_context *c, lr_poly *p0) {
    return guarded([&]() -> int { return rescale_one(c, p0, true, false); });
}
extern "C" int lr_div_floor_by_last_modulus(lr_context *c, lr_poly *p0) {
    return guarded([&]() -> int { return rescale_one(c, p0, false, false); });
}
extern "C" int lr_div_round_by_last_modulus_ntt(lr_context *c, lr_poly *p0) {
    return guarded([&]() -> int { return rescale_one(c, p0, true, true); });
}
extern "C" int lr_div_round_by_last_modulus(lr_context *c, lr_poly *p0) {
    return guarded([&]() -> int { return rescale_one(c, p0, false, true); });
}

static int rescale_many(lr_context *c, lr_poly *p0, int nb, int ntt_domain, bool round) {
    LR_TRY(check_rescale(c, p0));
    if (nb < 0 || nb >= p0->limbs) return fail(LR_ERR_SHAPE, "nbRescales must be below the limb count");
    LR_HIP(hipSetDevice(c->device));
    Rows r = rows_of(p0);
    if (ntt_domain) LR_TRY(run_ntt(c, true, r, r, 0, 1, p0->limbs, p0->batch));   // :59 / :154
    for (int k = 0; k < nb; ++k) LR_TRY(rescale_coeff_domain(c, p0, round));
    if (ntt_domain) LR_TRY(run_ntt(c, false, r, r, 0, 1, p0->limbs, p0->batch));  // :61 / :156
    return LR_OK;
}
extern "C" int lr_div_floor_by_last_modulus_many(lr_context *c, lr_poly *p0, int nb, int ntt_domain) {
    return guarded([&]() -> int {
    return rescale_many(c, p0, nb, ntt_domain, false);
    });
}
extern "C" int lr_div_round_by_last_modulus_many(lr_context *c, lr_poly *p0, int nb, int ntt_domain) {
    return guarded([&]() -> int {
    return rescale_many(c, p0, nb, ntt_domain, true);
    });
}

// diagnostics: the basis extension's division by a table constant (lr_bext.hip: div_by_const) against the IEEE division of
// ring/ring_basis_extension.go:372 on `samples` pseudo-random and adversarial operand pairs; *mismatches must come back 0
extern "C" int lr_selftest_division(lr_context *c, uint64_t samples, uint64_t seed, uint64_t *mismatches) {
    return guarded([&]() -> int {
        if (!c || !mismatches) return fail(LR_ERR_ARG, "null argument");
        LR_HIP(hipSetDevice(c->device));
        unsigned long long *d = nullptr;
        LR_HIP(hipMalloc((void **)&d, sizeof(unsigned long long)));
        const int per_thread = 4096;
        const int blocks = (int)std::min<uint64_t>(std::max<uint64_t>(1, samples / (256ull * per_thread)), 1u << 20);
        hipError_t e = hipMemsetAsync(d, 0, sizeof(unsigned long long), c->stream);
        if (e == hipSuccess) e = launch_div_selftest(seed, blocks, per_thread, d, c->stream);
        unsigned long long h = 0;
        if (e == hipSuccess) e = hipMemcpyAsync(&h, d, sizeof h, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        (void)hipFree(d);
        LR_HIP(e);
        *mismatches = h;
        return LR_OK;
    });
}

extern "C" int lr_context_timeline(lr_context *c, uint32_t *dst, size_t capacity, size_t *count) {
    return guarded([&]() -> int {
    if (!c || !count) return fail(LR_ERR_ARG, "null argument");
    *count = c->stamp_used;
    if (!dst) return LR_OK;                                   // size query
    if (capacity < c->stamp_used) return fail(LR_ERR_SHAPE, "timeline: destination too small");
    LR_HIP(hipSetDevice(c->device));
    LR_HIP(hipStreamSynchronize(c->stream));
    if (c->stamp_used) LR_HIP(hipMemcpy(dst, c->d_stamps, c->stamp_used * sizeof(u32), hipMemcpyDeviceToHost));
    return LR_OK;
    });
}

extern "C" int lr_context_last_ntt_kernel(const lr_context *c, char *buf, size_t capacity) {
    return guarded([&]() -> int {
    if (!c || !buf || capacity == 0) return fail(LR_ERR_ARG, "null argument");
    std::lock_guard<std::mutex> lock(c->diag_mu);
    std::snprintf(buf, capacity, "%s", c->last_ntt_kernel);
    return LR_OK;
    });
}
