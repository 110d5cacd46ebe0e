"""Host-side mirror of Lattigo's ``ring`` package over the C ABI (include/lattigo_ring.h).

Same exported names, argument order and meaning as the reference (github.com/ldsec/lattigo/ring,
v1.3.1) so that code and tests written against ``ring.Context`` read the same:

    ctx = ring.NewContextWithParams(N, moduli)      # ring/ring_context.go:60
    p = ctx.NewPoly()                               # ring/ring_context.go:288
    ctx.NTT(p, p)                                   # ring/ntt.go:4
    ctx.MulCoeffsMontgomery(a, b, c)                # ring/ring.go:221

Differences forced by the device boundary: a ``Poly`` is a *batch* of polynomials resident in
HBM ((poly, limb, coeff)-major uint64); ``Poly.set``/``Poly.get`` move numpy arrays of shape
[batch, limbs, N] (or [limbs, N] when batch == 1).  Errors the reference reports by panicking
are raised as ``LatticeRingError``.
"""
import ctypes as C

import numpy as np

from . import _native as nat
from ._native import LatticeRingError, Options, check, lib

# lr_ewise_op (include/lattigo_ring.h)
OPS = ["ADD", "ADD_NOMOD", "SUB", "SUB_NOMOD", "NEG", "REDUCE", "MUL_COEFFS", "MUL_COEFFS_AND_ADD",
       "MUL_COEFFS_AND_ADD_NOMOD", "MUL_COEFFS_CONSTANT", "MUL_MONT", "MUL_MONT_AND_ADD",
       "MUL_MONT_AND_ADD_NOMOD", "MUL_MONT_CONSTANT_AND_ADD_NOMOD", "MUL_MONT_AND_SUB",
       "MUL_MONT_AND_SUB_NOMOD", "MUL_MONT_CONSTANT", "MFORM", "INV_MFORM", "MUL_SCALAR",
       "MUL_SCALAR_LIMBS", "ADD_SCALAR_LIMBS", "SUB_SCALAR_LIMBS", "COPY", "MUL_BY_POW2"]
OP = {n: i for i, n in enumerate(OPS)}

TAB = {"MODULUS": 0, "BRED": 1, "MRED": 2, "PSI_MONT": 3, "PSI_INV_MONT": 4, "NTT_PSI": 5, "NTT_PSI_INV": 6,
       "NTT_N_INV": 7, "RESCALE": 8, "MASK": 9}


def _u64(vals):
    vals = [int(v) for v in vals]
    return (C.c_uint64 * len(vals))(*vals)


class Poly:
    """ring.Poly (ring/ring_object.go:11-13), as a device-resident batch."""

    def __init__(self, ctx, limbs, batch=1, _handle=None):
        self.ctx = ctx
        self.N = ctx.N
        self.alloc_limbs = limbs
        self.batch = batch
        if _handle is None:
            h = C.c_void_p()
            check(lib().lr_poly_alloc(ctx.h, limbs, batch, C.byref(h)))
            _handle = h
        self.h = _handle

    @classmethod
    def wrap(cls, ctx, device_ptr, limbs, batch):
        """A Poly over caller-owned device memory (e.g. a torch int64 tensor's data_ptr()), no copy (lr_poly_wrap)."""
        h = C.c_void_p()
        check(lib().lr_poly_wrap(ctx.h, C.c_void_p(device_ptr), limbs, batch, C.byref(h)))
        return cls(ctx, limbs, batch, _handle=h)

    @classmethod
    def wrap_strided(cls, ctx, device_ptr, limbs, batch, stride_limbs):
        """the same with `stride_limbs` limbs between consecutive polys (lr_poly_wrap_strided)"""
        h = C.c_void_p()
        check(lib().lr_poly_wrap_strided(ctx.h, C.c_void_p(device_ptr), limbs, batch, stride_limbs * ctx.N, C.byref(h)))
        return cls(ctx, limbs, batch, _handle=h)

    # --- reference accessors -----------------------------------------------------------
    def GetLenModuli(self):  # ring/ring_object.go:55
        n = C.c_int()
        check(lib().lr_poly_info(self.h, None, C.byref(n), None, None))
        return n.value

    def GetDegree(self):  # ring/ring_object.go:50
        return self.N

    def Zero(self):  # ring/ring_object.go:60
        check(lib().lr_poly_zero(self.h))

    @property
    def limbs(self):
        return self.GetLenModuli()

    @property
    def device_ptr(self):
        p = C.c_void_p()
        check(lib().lr_poly_info(self.h, None, None, None, C.byref(p)))
        return p.value

    # --- data movement -----------------------------------------------------------------
    def set(self, arr):
        a = np.ascontiguousarray(arr, dtype=np.uint64)
        limbs = self.limbs
        if a.ndim == 2:
            a = a[None]
        if a.shape != (self.batch, limbs, self.N):
            raise LatticeRingError(3, "expected shape %s, got %s" % ((self.batch, limbs, self.N), a.shape))
        check(lib().lr_poly_upload_dense(self.h, a.ctypes.data_as(C.c_void_p), a.size))
        return self

    def get(self):
        limbs = self.limbs
        out = np.empty((self.batch, limbs, self.N), dtype=np.uint64)
        check(lib().lr_poly_download_dense(self.h, out.ctypes.data_as(C.c_void_p), out.size))
        return out[0] if self.batch == 1 else out

    def UnmarshalBinary(self, data, batch_index=0):
        """Poly.UnmarshalBinary (ring/ring_object.go:252): the big-endian image goes to the device as it is."""
        data = bytes(data)
        check(lib().lr_poly_unmarshal(self.h, batch_index, data, len(data)))
        return self

    def MarshalBinary(self, batch_index=0):
        """Poly.MarshalBinary (ring/ring_object.go:222)."""
        buf = (C.c_uint8 * (2 + 8 * self.limbs * self.N))()
        n = C.c_size_t(0)
        check(lib().lr_poly_marshal(self.h, batch_index, buf, len(buf), C.byref(n)))
        return bytes(buf[:n.value])

    def set_limb_slices(self, batch_index, limb_arrays):
        """Go boundary form: one independent array per limb (``[][]uint64``)."""
        arrs = [np.ascontiguousarray(x, dtype=np.uint64) for x in limb_arrays]
        ptrs = (nat.u64p * len(arrs))(*[x.ctypes.data_as(nat.u64p) for x in arrs])
        check(lib().lr_poly_upload(self.h, batch_index, ptrs, len(arrs)))

    def get_limb_slices(self, batch_index, limbs=None):
        limbs = self.limbs if limbs is None else limbs
        arrs = [np.empty(self.N, dtype=np.uint64) for _ in range(limbs)]
        ptrs = (nat.u64p * limbs)(*[x.ctypes.data_as(nat.u64p) for x in arrs])
        check(lib().lr_poly_download(self.h, batch_index, ptrs, limbs))
        return arrs

    def CopyNew(self):  # ring/ring_object.go:67
        p = Poly(self.ctx, self.alloc_limbs, self.batch)
        check(lib().lr_poly_set_limbs(p.h, self.limbs))
        self.ctx._ew("COPY", self.limbs - 1, self, None, p)
        return p

    def __del__(self):
        try:
            if getattr(self, "h", None):
                lib().lr_poly_free(self.h)
                self.h = None
        except Exception:
            pass


class Context:
    """ring.Context (ring/ring_context.go:18-51)."""

    def __init__(self, N, Moduli, device=0, options=None):
        self.N = int(N)
        self.Modulus = [int(m) for m in Moduli]
        self.device = device
        h = C.c_void_p()
        if options is None:
            check(lib().lr_context_create(self.N, _u64(self.Modulus), len(self.Modulus), device, C.byref(h)))
        else:
            check(lib().lr_context_create_ex(self.N, _u64(self.Modulus), len(self.Modulus), device, C.byref(options), C.byref(h)))
        self.h = h

    def GetOptions(self):
        """the lr_options this context ended up with (after the test-only LR_* override), as an Options"""
        o = Options()
        check(lib().lr_context_get_options(self.h, C.byref(o)))
        return o

    def __del__(self):
        try:
            if getattr(self, "h", None):
                lib().lr_context_destroy(self.h)
                self.h = None
        except Exception:
            pass

    # --- getters (ring/ring_context.go:253-285) ----------------------------------------------
    def _table(self, name, shape):
        out = np.empty(shape, dtype=np.uint64)
        check(lib().lr_context_get_table(self.h, TAB[name], out.ctypes.data_as(nat.u64p), out.size))
        return out

    def GetBredParams(self):
        return self._table("BRED", (len(self.Modulus), 2))

    def GetMredParams(self):
        return self._table("MRED", (len(self.Modulus),))

    def GetPsi(self):
        return self._table("PSI_MONT", (len(self.Modulus),))

    def GetPsiInv(self):
        return self._table("PSI_INV_MONT", (len(self.Modulus),))

    def GetNttPsi(self):
        return self._table("NTT_PSI", (len(self.Modulus), self.N))

    def GetNttPsiInv(self):
        return self._table("NTT_PSI_INV", (len(self.Modulus), self.N))

    def GetNttNInv(self):
        return self._table("NTT_N_INV", (len(self.Modulus),))

    def GetRescaleParams(self):
        return self._table("RESCALE", (len(self.Modulus), len(self.Modulus)))

    def Sync(self):
        check(lib().lr_context_sync(self.h))

    def SetStream(self, stream_ptr):
        """an externally owned hipStream_t handle, or None for the library's own stream.  Handle 0 is HIP's legacy default stream,
        which the C ABI cannot express (NULL there selects the library's stream, and that one does not synchronise with the legacy
        stream): it is refused here instead of silently running somewhere else than the caller thinks."""
        if stream_ptr is None:
            check(lib().lr_context_set_stream(self.h, C.c_void_p(None)))
            return
        if int(stream_ptr) == 0:
            raise LatticeRingError(1, "SetStream(0): the legacy default stream cannot be selected; create an explicit stream "
                                      "(torch.cuda.Stream()) and pass its handle, or None for the library's own stream")
        check(lib().lr_context_set_stream(self.h, C.c_void_p(int(stream_ptr))))

    # --- allocation (ring/ring_context.go:288,300) -------------------------------------------
    def NewPoly(self, batch=1):
        return Poly(self, len(self.Modulus), batch)

    def NewPolyLvl(self, level, batch=1):
        return Poly(self, level + 1, batch)

    # --- NTT (ring/ntt.go:4-29) ---------------------------------------------------------------
    def NTT(self, p1, p2):
        check(lib().lr_ntt(self.h, len(self.Modulus) - 1, p1.h, p2.h))

    def NTTLvl(self, level, p1, p2):
        check(lib().lr_ntt(self.h, level, p1.h, p2.h))

    def InvNTT(self, p1, p2):
        check(lib().lr_intt(self.h, len(self.Modulus) - 1, p1.h, p2.h))

    def InvNTTLvl(self, level, p1, p2):
        check(lib().lr_intt(self.h, level, p1.h, p2.h))

    def NTTLimb(self, mod_index, p1, limb1, p2, limb2):  # package-level ring.NTT (ring/ntt.go:53)
        check(lib().lr_ntt_limb(self.h, mod_index, p1.h, limb1, p2.h, limb2))

    def InvNTTLimb(self, mod_index, p1, limb1, p2, limb2):  # ring.InvNTT (ring/ntt.go:89)
        check(lib().lr_intt_limb(self.h, mod_index, p1.h, limb1, p2.h, limb2))

    def NTTHost(self, limb_arrays):
        """Literal Go call shape: per-limb host slices in, per-limb host slices out."""
        ins = [np.ascontiguousarray(x, dtype=np.uint64) for x in limb_arrays]
        outs = [np.empty(self.N, dtype=np.uint64) for _ in ins]
        pi = (nat.u64p * len(ins))(*[x.ctypes.data_as(nat.u64p) for x in ins])
        po = (nat.u64p * len(ins))(*[x.ctypes.data_as(nat.u64p) for x in outs])
        check(lib().lr_ntt_host(self.h, len(ins) - 1, pi, po))
        return outs

    def InvNTTHost(self, limb_arrays):
        ins = [np.ascontiguousarray(x, dtype=np.uint64) for x in limb_arrays]
        outs = [np.empty(self.N, dtype=np.uint64) for _ in ins]
        pi = (nat.u64p * len(ins))(*[x.ctypes.data_as(nat.u64p) for x in ins])
        po = (nat.u64p * len(ins))(*[x.ctypes.data_as(nat.u64p) for x in outs])
        check(lib().lr_intt_host(self.h, len(ins) - 1, pi, po))
        return outs

    # --- coefficient-wise family (ring/ring.go) ------------------------------------------------
    def _ew(self, op, level, a, b, out, scalars=None):
        sc = None if scalars is None else _u64(scalars)
        check(lib().lr_ewise(self.h, OP[op], level, a.h, None if b is None else b.h, out.h, sc))

    def _full(self):
        return len(self.Modulus) - 1

    def Add(self, p1, p2, p3): self._ew("ADD", self._full(), p1, p2, p3)
    def AddLvl(self, level, p1, p2, p3): self._ew("ADD", level, p1, p2, p3)
    def AddNoMod(self, p1, p2, p3): self._ew("ADD_NOMOD", self._full(), p1, p2, p3)
    def AddNoModLvl(self, level, p1, p2, p3): self._ew("ADD_NOMOD", level, p1, p2, p3)
    def Sub(self, p1, p2, p3): self._ew("SUB", self._full(), p1, p2, p3)
    def SubLvl(self, level, p1, p2, p3): self._ew("SUB", level, p1, p2, p3)
    def SubNoMod(self, p1, p2, p3): self._ew("SUB_NOMOD", self._full(), p1, p2, p3)
    def SubNoModLvl(self, level, p1, p2, p3): self._ew("SUB_NOMOD", level, p1, p2, p3)
    def Neg(self, p1, p2): self._ew("NEG", self._full(), p1, None, p2)
    def NegLvl(self, level, p1, p2): self._ew("NEG", level, p1, None, p2)
    def Reduce(self, p1, p2): self._ew("REDUCE", self._full(), p1, None, p2)
    def ReduceLvl(self, level, p1, p2): self._ew("REDUCE", level, p1, None, p2)
    def MulCoeffs(self, p1, p2, p3): self._ew("MUL_COEFFS", self._full(), p1, p2, p3)
    def MulCoeffsAndAdd(self, p1, p2, p3): self._ew("MUL_COEFFS_AND_ADD", self._full(), p1, p2, p3)
    def MulCoeffsAndAddNoMod(self, p1, p2, p3): self._ew("MUL_COEFFS_AND_ADD_NOMOD", self._full(), p1, p2, p3)
    def MulCoeffsConstant(self, p1, p2, p3): self._ew("MUL_COEFFS_CONSTANT", self._full(), p1, p2, p3)
    def MulCoeffsMontgomery(self, p1, p2, p3): self._ew("MUL_MONT", self._full(), p1, p2, p3)
    def MulCoeffsMontgomeryLvl(self, level, p1, p2, p3): self._ew("MUL_MONT", level, p1, p2, p3)
    def MulCoeffsMontgomeryAndAdd(self, p1, p2, p3): self._ew("MUL_MONT_AND_ADD", self._full(), p1, p2, p3)
    def MulCoeffsMontgomeryAndAddLvl(self, level, p1, p2, p3): self._ew("MUL_MONT_AND_ADD", level, p1, p2, p3)
    def MulCoeffsMontgomeryAndAddNoMod(self, p1, p2, p3): self._ew("MUL_MONT_AND_ADD_NOMOD", self._full(), p1, p2, p3)
    def MulCoeffsMontgomeryAndAddNoModLvl(self, level, p1, p2, p3): self._ew("MUL_MONT_AND_ADD_NOMOD", level, p1, p2, p3)
    def MulCoeffsMontgomeryConstantAndAddNoModLvl(self, level, p1, p2, p3):
        self._ew("MUL_MONT_CONSTANT_AND_ADD_NOMOD", level, p1, p2, p3)
    def MulCoeffsMontgomeryAndSub(self, p1, p2, p3): self._ew("MUL_MONT_AND_SUB", self._full(), p1, p2, p3)
    def MulCoeffsMontgomeryAndSubNoMod(self, p1, p2, p3): self._ew("MUL_MONT_AND_SUB_NOMOD", self._full(), p1, p2, p3)
    def MulCoeffsMontgomeryConstant(self, p1, p2, p3): self._ew("MUL_MONT_CONSTANT", self._full(), p1, p2, p3)
    def MForm(self, p1, p2): self._ew("MFORM", self._full(), p1, None, p2)
    def MFormLvl(self, level, p1, p2): self._ew("MFORM", level, p1, None, p2)
    def InvMForm(self, p1, p2): self._ew("INV_MFORM", self._full(), p1, None, p2)
    def MulScalar(self, p1, scalar, p2): self._ew("MUL_SCALAR", self._full(), p1, None, p2, [scalar])
    def MulScalarLvl(self, level, p1, scalar, p2): self._ew("MUL_SCALAR", level, p1, None, p2, [scalar])
    def Copy(self, p0, p1): self._ew("COPY", self._full(), p0, None, p1)
    def CopyLvl(self, level, p0, p1): self._ew("COPY", level, p0, None, p1)
    def MulByPow2(self, p1, pow2, p2): self._ew("MUL_BY_POW2", self._full(), p1, None, p2, [pow2])
    def MulByPow2Lvl(self, level, p1, pow2, p2): self._ew("MUL_BY_POW2", level, p1, None, p2, [pow2])

    def MulScalarBigint(self, p1, scalar, p2):  # ring/ring.go:541
        self._ew("MUL_SCALAR_LIMBS", self._full(), p1, None, p2, [int(scalar) % q for q in self.Modulus])

    def MulScalarBigintLvl(self, level, p1, scalar, p2):  # ring/ring.go:557
        self._ew("MUL_SCALAR_LIMBS", level, p1, None, p2, [int(scalar) % q for q in self.Modulus[:level + 1]])

    def AddScalarBigint(self, p1, scalar, p2):
        # the reference writes into p1, not p2 (ring/ring.go:482: p1tmp, p2tmp := p1.Coeffs[i], p1.Coeffs[i])
        self._ew("ADD_SCALAR_LIMBS", self._full(), p1, None, p1, [int(scalar) % q for q in self.Modulus])

    def SubScalarBigint(self, p1, scalar, p2):  # ring/ring.go:500, same quirk
        self._ew("SUB_SCALAR_LIMBS", self._full(), p1, None, p1, [int(scalar) % q for q in self.Modulus])

    def MulPolyMontgomery(self, p1, p2, p3):  # ring/ring.go:370
        a, b = self.NewPoly(p1.batch), self.NewPoly(p1.batch)
        self.NTT(p1, a)
        self.NTT(p2, b)
        self.MulCoeffsMontgomery(a, b, p3)
        self.InvNTT(p3, p3)

    # --- Galois automorphisms (ring/ring_galois.go) ------------------------------------------------
    def Permute(self, polIn, gen, polOut):  # :106
        check(lib().lr_permute(self.h, polIn.h, int(gen), polOut.h))

    def ntt_variants(self):
        """(forward, inverse) assembly variants this context selects (diagnostics)"""
        f, i = C.c_int(), C.c_int()
        check(lib().lr_context_ntt_variants(self.h, C.byref(f), C.byref(i)))
        return f.value, i.value

    def last_ntt_kernel(self):
        """name of the kernel the last NTT / InvNTT launch of this context dispatched (diagnostics)"""
        buf = C.create_string_buffer(64)
        check(lib().lr_context_last_ntt_kernel(self.h, buf, len(buf)))
        return buf.value.decode()

    def selftest_division(self, samples, seed=1):
        """diagnostics: quotients of the extension's constant-divisor division that differ from IEEE division (must be 0)"""
        n = C.c_uint64(0)
        check(lib().lr_selftest_division(self.h, samples, seed, C.byref(n)))
        return int(n.value)

    def timeline(self):
        """clock stamps of the last launch of the stamped diagnostics kernel (context created under LR_NTT_TIMELINE=1):
        uint32 array [workgroups, 16 waves, 16 stamps]"""
        n = C.c_size_t(0)
        check(lib().lr_context_timeline(self.h, None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=np.uint32)
        if n.value:
            check(lib().lr_context_timeline(self.h, out.ctypes.data_as(C.c_void_p), out.size, C.byref(n)))
        return out.reshape(-1, 16, 16)

    def HalfScalarOp(self, op, level, p1, lo, hi, p2):
        """the element loops of ckks.Evaluator's AddConst / MultByConst / MultByConstAndAdd / MultByi / DivByi (ckks/evaluator.go:429-828):
        op "ADD" CRed(x + s), "MRED" MRed(x, s), "MRED_ADD" CRed(out + MRed(x, s)); s = lo[i] below N/2, hi[i] above"""
        lo = np.ascontiguousarray(lo, dtype=np.uint64)
        hi = np.ascontiguousarray(hi, dtype=np.uint64)
        if lo.size < level + 1 or hi.size < level + 1:
            raise LatticeRingError(3, "half-vector scalars: need level+1 words each")
        check(lib().lr_half_scalar_op(self.h, {"ADD": 0, "MRED": 1, "MRED_ADD": 2}[op], level, p1.h, lo.ctypes.data_as(C.c_void_p),
                                      hi.ctypes.data_as(C.c_void_p), p2.h))

    def CkksLinComb(self, level, terms, consts, add=None, accumulate=False, out=None):
        """res = c0 + sum c_k ct_k on both components of degree-1 ciphertexts in one device call (lr_ckks_lincomb): the element loops of
        evaluatePolyFromPowerBasis' chain (ckks/polynomial_evaluation.go:142-159), AddConst once and per term MultByConst on the receiver
        where the reference equalises scales and MultByConstAndAdd, in the terms' order.  terms: [(c0, c1), ...] Polys; consts: a
        CkksLinCombConsts (ckks_lincomb_constants) or anything with has_pre [T], pre / lo / hi [T][level+1]; add: (add_lo, add_hi) of
        level+1 words each, or None; accumulate: on top of the receiver instead of zero; out: (out0, out1).  The same bits as HalfScalarOp
        "ADD", then per term "MRED" and "MRED_ADD"."""
        T, L1 = len(terms), level + 1

        def words(a, n, what, dtype=np.uint64):
            a = np.ascontiguousarray(a, dtype=dtype).reshape(-1)
            if a.size != n:
                raise LatticeRingError(3, "CkksLinComb: need %d words in %s" % (n, what))
            return a
        has_pre = words(consts.has_pre, T, "has_pre", np.uint8)
        pre, lo, hi = (words(getattr(consts, n), T * L1, n) for n in ("pre", "lo", "hi"))
        a_lo, a_hi = (None, None) if add is None else (words(add[0], L1, "add_lo"), words(add[1], L1, "add_hi"))
        ptr = lambda a: None if a is None or a.size == 0 else a.ctypes.data_as(C.c_void_p)
        t0 = (C.c_void_p * max(T, 1))(*[t[0].h.value for t in terms])
        t1 = (C.c_void_p * max(T, 1))(*[t[1].h.value for t in terms])
        check(lib().lr_ckks_lincomb(self.h, level, T, t0, t1, ptr(has_pre), ptr(pre), ptr(lo), ptr(hi), ptr(a_lo), ptr(a_hi),
                                    1 if accumulate else 0, out[0].h, out[1].h))
        return out

    def CkksCombine(self, op, level, a, b, out, double_a=False, ma=None, mb=None, add=None):
        """out = a (+|-) b over CKKS ciphertexts of any degree in one device call (lr_ckks_combine): the element loops of evaluator.Add /
        AddNoMod / Sub / SubNoMod through evaluateInPlace (ckks/evaluator.go:227-342) with Sub's NegLvl tail, and the steps of the same
        shape between the products of the Chebyshev drivers.  op: "ADD", "ADD_NOMOD", "SUB" or "SUB_NOMOD"; a, b, out: the components'
        Polys (b None: no b); out[u] may be a[u] or b[u].  double_a: x = CRed(x + x) first; ma / mb: the multiplier of a / b, either one
        array of level+1 words (ckks_combine_constants' mult) or (lo, hi); add: (add_lo, add_hi) for component 0, or None.  The same bits
        as the sequence of HalfScalarOp "MRED" / "ADD" and AddLvl .. NegLvl, CopyLvl calls."""
        L1 = level + 1

        def half_words(w, what):
            if w is None:
                return None, None
            lo, hi = w if isinstance(w, tuple) else (w, w)
            lo, hi = (np.ascontiguousarray(x, dtype=np.uint64).reshape(-1) for x in (lo, hi))
            if lo.size != L1 or hi.size != L1:
                raise LatticeRingError(3, "CkksCombine: need %d words in each half of %s" % (L1, what))
            return lo, hi
        words = [half_words(ma, "ma"), half_words(mb, "mb"), half_words(add, "add")]
        ptr = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)
        handles = lambda polys: (C.c_void_p * max(len(polys), 1))(*[p.h.value for p in polys])
        check(lib().lr_ckks_combine(self.h, {"ADD": 0, "ADD_NOMOD": 1, "SUB": 2, "SUB_NOMOD": 3}[op], level, len(a) - 1, handles(a),
                                    -1 if b is None else len(b) - 1, None if b is None else handles(b), 1 if double_a else 0,
                                    *[ptr(x) for pair in words for x in pair], handles(out)))
        return out

    def MultByMonomial(self, p1, monomialDeg, p2):  # ring/ring.go:663
        check(lib().lr_mult_by_monomial(self.h, p1.h, int(monomialDeg), p2.h))

    def Shift(self, p1, n, p2):  # ring/ring.go:575
        check(lib().lr_shift(self.h, p1.h, int(n), p2.h))

    def Rotate(self, p1, n, p2=None):  # ring/ring.go:775 -- the reference writes into p1 and ignores p2 (:791)
        check(lib().lr_rotate(self.h, p1.h, int(n)))

    def PermuteNTTLvl(self, level, polIn, gen, polOut):  # package-level PermuteNTT (:55) on limbs 0..level
        check(lib().lr_permute_ntt(self.h, level, polIn.h, int(gen), polOut.h))

    # --- RNS rescale (ring/ring_scaling.go:9-164) ----------------------------------------------
    def DivFloorByLastModulusNTT(self, p0): check(lib().lr_div_floor_by_last_modulus_ntt(self.h, p0.h))
    def DivFloorByLastModulus(self, p0): check(lib().lr_div_floor_by_last_modulus(self.h, p0.h))
    def DivRoundByLastModulusNTT(self, p0): check(lib().lr_div_round_by_last_modulus_ntt(self.h, p0.h))
    def DivRoundByLastModulus(self, p0): check(lib().lr_div_round_by_last_modulus(self.h, p0.h))
    def DivFloorByLastModulusMany(self, p0, nb): check(lib().lr_div_floor_by_last_modulus_many(self.h, p0.h, nb, 0))
    def DivFloorByLastModulusManyNTT(self, p0, nb): check(lib().lr_div_floor_by_last_modulus_many(self.h, p0.h, nb, 1))
    def DivRoundByLastModulusMany(self, p0, nb): check(lib().lr_div_round_by_last_modulus_many(self.h, p0.h, nb, 0))
    def DivRoundByLastModulusManyNTT(self, p0, nb): check(lib().lr_div_round_by_last_modulus_many(self.h, p0.h, nb, 1))

    # --- multi-device (one process, one thread per device): SURVEY 8(e) ---------------------------
    def CopyPeer(self, dst, dst_index, src_ctx, src, src_index, count):
        """polys [src_index, +count) of src (on src_ctx's device) -> slots [dst_index, ...) of dst (on this context's device), on the copy
        stream of that device pair, behind what src_ctx has enqueued so far (lr_poly_copy_peer); asynchronous"""
        check(lib().lr_poly_copy_peer(self.h, dst.h, dst_index, src_ctx.h, src.h, src_index, count))

    def WaitPeerCopies(self):
        """this context's stream waits (on the device) for every peer copy into its device enqueued so far"""
        check(lib().lr_context_wait_peer_copies(self.h))

    def GatherBlocks(self, dst, blocks):
        """blocks: [(src_ctx, src_poly, count)] -> dst, one behind the other in block order, then WaitPeerCopies (lr_gather_blocks)"""
        n = len(blocks)
        ctxs = (C.c_void_p * n)(*[b[0].h.value for b in blocks])
        polys = (C.c_void_p * n)(*[b[1].h.value for b in blocks])
        counts = (C.c_int * n)(*[int(b[2]) for b in blocks])
        check(lib().lr_gather_blocks(self.h, dst.h, ctxs, polys, counts, n))

    # --- measurement -------------------------------------------------------------------------
    def TimerStart(self):
        check(lib().lr_timer_start(self.h))

    def TimerStop(self):
        ms = C.c_float()
        check(lib().lr_timer_stop(self.h, C.byref(ms)))
        return ms.value


def GenGaloisParams(n, gen):
    """ring.GenGaloisParams (ring/ring_galois.go:9): powers of gen modulo 2n"""
    out, mask = [1], (n << 1) - 1
    for _ in range(1, n >> 1):
        out.append((out[-1] * gen) & mask)
    return out


def PermuteNTTIndex(gen, power, N):
    """ring.PermuteNTTIndex (ring/ring_galois.go:29)"""
    idx = np.empty(N, dtype=np.uint64)
    check(lib().lr_permute_ntt_index(int(gen), int(power), int(N), idx.ctypes.data_as(nat.u64p)))
    return idx


def PermuteNTT(context, polIn, gen, polOut):
    """ring.PermuteNTT (ring/ring_galois.go:55): all limbs of polIn"""
    context.PermuteNTTLvl(polIn.limbs - 1, polIn, gen, polOut)


class CkksLinCombConsts:
    """what ckks_lincomb_constants yields: level_after, scale_after, add = (add_lo, add_hi) or None, has_pre [T], pre / lo / hi
    [T][level_after + 1]"""

    def __init__(self, level_after, scale_after, add, has_pre, pre, lo, hi):
        self.level_after, self.scale_after, self.add = level_after, scale_after, add
        self.has_pre, self.pre, self.lo, self.hi = has_pre, pre, lo, hi


def ckks_lincomb_constants(moduli, ntt_psi1, default_scale, res_level, res_scale, terms, c0=None):
    """The scalar lines of res = c0 + sum c_k ct_k as the reference runs it (lr_ckks_lincomb_constants; evaluatePolyFromPowerBasis,
    ckks/polynomial_evaluation.go:142-159: AddConst(res, c0, res) if c0 is given, then MultByConstAndAdd(ct_k, c_k, res) in the terms'
    order, with the MultByConst calls on the receiver that equalise scales).  Host only: needs no context and no device.
    moduli, ntt_psi1: the moduli and per limb the word GetNttPsi()[i][1]; default_scale: ckksContext.scale; res_level, res_scale: the
    receiver before the chain; terms: [(constant, scale, level), ...] with complex (or real) constants.  Returns a CkksLinCombConsts."""
    moduli = [int(q) for q in moduli]
    L, T = len(moduli), len(terms)
    cs = [complex(t[0]) for t in terms]
    dbl = lambda vals: (C.c_double * max(len(vals), 1))(*[float(v) for v in vals])
    lv = (C.c_int * max(T, 1))(*[int(t[2]) for t in terms])
    level_after, scale_after = C.c_int(0), C.c_double(0.0)
    add_lo, add_hi = np.zeros(L, dtype=np.uint64), np.zeros(L, dtype=np.uint64)
    has_pre = np.zeros(max(T, 1), dtype=np.uint8)
    pre, lo, hi = (np.zeros(max(T * L, 1), dtype=np.uint64) for _ in range(3))
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    z = complex(c0) if c0 is not None else 0j
    check(lib().lr_ckks_lincomb_constants(_u64(moduli), _u64(ntt_psi1), L, float(default_scale), int(res_level), float(res_scale),
                                          0 if c0 is None else 1, z.real, z.imag, T, dbl([c.real for c in cs]), dbl([c.imag for c in cs]),
                                          dbl([t[1] for t in terms]), lv, C.byref(level_after), C.byref(scale_after), ptr(add_lo), ptr(add_hi),
                                          ptr(has_pre), ptr(pre), ptr(lo), ptr(hi)))
    L1 = level_after.value + 1
    rows = lambda a: a[:T * L1].reshape(T, L1).copy()
    return CkksLinCombConsts(level_after.value, scale_after.value, None if c0 is None else (add_lo[:L1].copy(), add_hi[:L1].copy()),
                             has_pre[:T].copy(), rows(pre), rows(lo), rows(hi))


class CkksCombineConsts:
    """what ckks_combine_constants yields: level_after, scale_after, degree_after, mult_side (0 none, 1 a, 2 b) and mult [level_after + 1]
    (None when nothing is multiplied)"""

    def __init__(self, level_after, scale_after, degree_after, mult_side, mult):
        self.level_after, self.scale_after, self.degree_after, self.mult_side, self.mult = level_after, scale_after, degree_after, mult_side, mult


CKKS_COMBINE_RECEIVER = {"new": 0, "a": 1, "b": 2, "both": 3}


def ckks_combine_constants(moduli, op, a, b, out, receiver="new"):
    """The scalar lines of evaluator.Add / AddNoMod / Sub / SubNoMod as the reference runs them (lr_ckks_combine_constants;
    evaluateInPlace, ckks/evaluator.go:227-342, and its callers' degree rules).  Host only: needs no context and no device.
    op: "ADD", "ADD_NOMOD", "SUB" or "SUB_NOMOD"; a, b, out: (degree, level, scale) of the operands and of the receiver before the call;
    receiver: "new", "a", "b" or "both" (a is b is the receiver).  Returns a CkksCombineConsts; raises LatticeRingError where the
    reference panics (LR_ERR_UNSUPPORTED) and outside the domain (LR_ERR_ARG)."""
    moduli = [int(q) for q in moduli]
    level_after, degree_after, mult_side, scale_after = C.c_int(0), C.c_int(0), C.c_int(0), C.c_double(0.0)
    mult = np.zeros(max(len(moduli), 1), dtype=np.uint64)
    check(lib().lr_ckks_combine_constants(_u64(moduli), len(moduli), {"ADD": 0, "ADD_NOMOD": 1, "SUB": 2, "SUB_NOMOD": 3}[op], int(a[0]), int(a[1]),
                                          float(a[2]), int(b[0]), int(b[1]), float(b[2]), int(out[0]), int(out[1]), float(out[2]),
                                          CKKS_COMBINE_RECEIVER[receiver], C.byref(level_after), C.byref(scale_after), C.byref(degree_after),
                                          C.byref(mult_side), mult.ctypes.data_as(C.c_void_p)))
    return CkksCombineConsts(level_after.value, scale_after.value, degree_after.value, mult_side.value,
                             mult[:level_after.value + 1].copy() if mult_side.value else None)


class CkksBasisSchedule:
    """what ckks_power_basis_schedule yields: products (a list of _native.BasisProduct in the reference's order of creation), mult and
    add [len(products)][len(moduli)] (the words of the Chebyshev tails, zero where unused), and index: n -> position in products"""

    def __init__(self, products, mult, add):
        self.products, self.mult, self.add = products, mult, add
        self.index = {int(p.n): k for k, p in enumerate(products)}

    def level(self, n, c1_level):
        return c1_level if n == 1 else self.products[self.index[n]].level_after


def ckks_power_basis_targets(degree, fast=True):
    """The n of the computePowerBasis / computePowerBasisCheby calls of EvaluateChebyFast / EvaluatePolyFast (fast) or EvaluateChebyEco /
    EvaluatePolyEco for a polynomial of that degree, in their order (ckks/chebyshev_evaluation.go:20-29, :46-55;
    ckks/polynomial_evaluation.go:17-26, :42-51): 2 .. 2^L, then 2^i for L < i < M, with M = bits.Len64(degree - 1), L = M >> 1 or 1."""
    M = (int(degree) - 1).bit_length()
    L = M >> 1 if fast else 1
    return list(range(2, (1 << L) + 1)) + [1 << i for i in range(L + 1, M)]


def ckks_power_basis_schedule(moduli, default_scale, chebyshev, c1_level, c1_scale, targets):
    """The scalar lines of the power basis as the reference runs it (lr_ckks_power_basis_schedule; computePowerBasis,
    ckks/polynomial_evaluation.go:76-93, computePowerBasisCheby, ckks/chebyshev_evaluation.go:60-101): which products, and per product
    the level, Rescale's trip count, the scale and the words of the Chebyshev tail.  Host only: needs no context and no device.
    targets: the n of the caller's computePowerBasis(n) calls, in order (ckks_power_basis_targets).  Returns a CkksBasisSchedule."""
    moduli = [int(q) for q in moduli]
    L, T = len(moduli), len(targets)
    if any(not 1 <= int(t) <= 65535 for t in targets):      # before the narrowing to 32 bits, which would wrap
        raise LatticeRingError(4, "CKKS power basis schedule: a target is 0 or above 65535")
    tg = (C.c_uint32 * max(T, 1))(*[int(t) for t in targets])
    count = C.c_int(-1)
    args = (_u64(moduli), L, float(default_scale), 1 if chebyshev else 0, int(c1_level), float(c1_scale), T, tg)
    rc = lib().lr_ckks_power_basis_schedule(*args, 0, C.byref(count), None, None, None)
    if rc != 0 and count.value < 0:
        check(rc)
    n = max(count.value, 0)
    products = (nat.BasisProduct * max(n, 1))()
    mult, add = np.zeros((max(n, 1), L), dtype=np.uint64), np.zeros((max(n, 1), L), dtype=np.uint64)
    check(lib().lr_ckks_power_basis_schedule(*args, n, C.byref(count), products, mult.ctypes.data_as(C.c_void_p), add.ctypes.data_as(C.c_void_p)))
    return CkksBasisSchedule([products[k] for k in range(count.value)], mult[:count.value].copy(), add[:count.value].copy())


def NewContextWithParams(N, Moduli, device=0, options=None):
    """ring.NewContextWithParams (ring/ring_context.go:60).  Raises LatticeRingError
    LR_ERR_NOT_NTT_FRIENDLY where the reference returns its error value.  options: an Options (lr_options) or None for the defaults."""
    return Context(N, Moduli, device, options)


class FastBasisExtender:
    """ring.FastBasisExtender (ring/ring_basis_extension.go:9-74)."""

    def __init__(self, contextQ, contextP):
        self.contextQ, self.contextP = contextQ, contextP
        h = C.c_void_p()
        check(lib().lr_bext_create(contextQ.h, contextP.h, C.byref(h)))
        self.h = h

    def __del__(self):
        try:
            if getattr(self, "h", None):
                lib().lr_bext_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def ModDownParamsPQ(self):
        out = np.empty(len(self.contextQ.Modulus), dtype=np.uint64)
        check(lib().lr_bext_get_table(self.h, 0, out.ctypes.data_as(nat.u64p), out.size))
        return out

    def ModDownParamsQP(self):
        out = np.empty(len(self.contextP.Modulus), dtype=np.uint64)
        check(lib().lr_bext_get_table(self.h, 1, out.ctypes.data_as(nat.u64p), out.size))
        return out

    def ModUpSplitQP(self, level, p1, p2): check(lib().lr_modup_split_qp(self.h, level, p1.h, p2.h))
    def ModUpSplitPQ(self, level, p1, p2): check(lib().lr_modup_split_pq(self.h, level, p1.h, p2.h))
    def ModDownNTTPQ(self, level, p1, p2): check(lib().lr_moddown_ntt_pq(self.h, level, p1.h, p2.h))
    def ModDownSplitedNTTPQ(self, level, p1Q, p1P, p2): check(lib().lr_moddown_split_ntt_pq(self.h, level, p1Q.h, p1P.h, p2.h))
    def ModDownPQ(self, level, p1, p2): check(lib().lr_moddown_pq(self.h, level, p1.h, p2.h))
    def ModDownSplitedPQ(self, level, p1Q, p1P, p2): check(lib().lr_moddown_split_pq(self.h, level, p1Q.h, p1P.h, p2.h))
    def ModDownSplitedQP(self, levelQ, levelP, p1Q, p1P, p2):
        check(lib().lr_moddown_split_qp(self.h, levelQ, levelP, p1Q.h, p1P.h, p2.h))


def NewFastBasisExtender(contextQ, contextP):
    return FastBasisExtender(contextQ, contextP)


class Decomposer:
    """ring.Decomposer (ring/ring_basis_extension.go:398-472).  The reference constructor takes the
    modulus lists; here the two contexts (which carry them) so the handle knows its device."""

    def __init__(self, contextQ, contextP):
        self.contextQ, self.contextP = contextQ, contextP
        h = C.c_void_p()
        check(lib().lr_decomposer_create(contextQ.h, contextP.h, C.byref(h)))
        self.h = h
        nQ, nP = len(contextQ.Modulus), len(contextP.Modulus)
        self.alpha = nP
        self.beta = -(-nQ // nP)
        self.xalpha = [nP] * self.beta
        if nQ % nP:
            self.xalpha[-1] = nQ % nP

    def __del__(self):
        try:
            if getattr(self, "h", None):
                lib().lr_decomposer_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def Xalpha(self):
        return list(self.xalpha)

    def Decompose(self, level, crtDecompLevel, p0, p1):
        check(lib().lr_decompose(self.h, level, crtDecompLevel, p0.h, p1.h))

    def DecomposeAndSplit(self, level, crtDecompLevel, p0, p1Q, p1P):
        check(lib().lr_decompose_and_split(self.h, level, crtDecompLevel, p0.h, p1Q.h, p1P.h))


def NewDecomposer(contextQ, contextP):
    return Decomposer(contextQ, contextP)


class SimpleScaler:
    """ring.SimpleScaler (ring/ring_scaling.go:168-300): reconstruct a polynomial of `context`, scale it by t/Q and
    return it modulo t."""

    def __init__(self, t, context):
        self.t, self.context = int(t), context
        h = C.c_void_p()
        check(lib().lr_simple_scaler_create(context.h, self.t, C.byref(h)))
        self.h = h

    def __del__(self):
        try:
            if getattr(self, "h", None):
                lib().lr_simple_scaler_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def tables(self):
        """(wi[L], ti[L][2]) as computed on the host by NewSimpleScaler"""
        n = len(self.context.Modulus)
        wi = np.zeros(n, dtype=np.uint64)
        ti = np.zeros((n, 2), dtype=np.float64)
        check(lib().lr_simple_scaler_tables(self.h, wi.ctypes.data_as(C.POINTER(C.c_uint64)), ti.ctypes.data_as(C.POINTER(C.c_double)), n))
        return wi, ti

    def Scale(self, p1, p2):  # :275
        check(lib().lr_simple_scale(self.h, p1.h, p2.h))


def NewSimpleScaler(t, context):  # ring/ring_scaling.go:186
    return SimpleScaler(t, context)


class CkksPlan:
    """What ckks.NewEvaluator builds around the ring (ckks/evaluator.go:81-112) plus the
    MulRelin / switchKeysInPlace / Rescale call sequences (:1016, :1475, :933), device-resident."""

    def __init__(self, contextQ, contextP, max_batch=1, options=None):
        self.contextQ, self.contextP = contextQ, contextP
        h = C.c_void_p()
        if options is None:
            check(lib().lr_ckks_plan_create(contextQ.h, contextP.h, max_batch, C.byref(h)))
        else:
            check(lib().lr_ckks_plan_create_ex(contextQ.h, contextP.h, max_batch, C.byref(options), C.byref(h)))
        self.h = h

    def __del__(self):
        try:
            if getattr(self, "h", None):
                lib().lr_ckks_plan_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def Stats(self):
        """diagnostics: forks (independent launches of a small batch side by side), grouped digit extensions (lr_ckks_plan_stats)"""
        f, g = C.c_uint64(), C.c_uint64()
        check(lib().lr_ckks_plan_stats(self.h, C.byref(f), C.byref(g)))
        return {"forks": f.value, "grouped_extensions": g.value}

    def NewSwitchingKey(self, batch=1):
        """Storage for SwitchingKey.evakey (ckks/keygen.go:68-70): beta x 2 polys over Q||P."""
        nQ, nP = len(self.contextQ.Modulus), len(self.contextP.Modulus)
        beta = -(-nQ // nP)
        return Poly(self.contextQ, nQ + nP, 2 * beta)

    def SwitchKeysInPlace(self, level, cx, evakey, p0, p1):
        check(lib().lr_ckks_switch_keys(self.h, level, cx.h, evakey.h, p0.h, p1.h))

    # bfv.NewEvaluator builds the same objects for its key switch (decomposer, baseconverterQ1P, pools: bfv/evaluator.go:100-112):
    # one plan over (contextQ, contextP) serves both schemes
    def BfvSwitchKeys(self, cx, evakey, p0, p1):
        """bfv.evaluator.switchKeys (bfv/evaluator.go:736): coefficient domain in and out, all of Q"""
        check(lib().lr_bfv_switch_keys(self.h, cx.h, evakey.h, p0.h, p1.h))

    def BfvRelinearize(self, ct, evakey, ctOut):
        """bfv.evaluator.Relinearize (bfv/evaluator.go:512) of a degree-2 ciphertext: ct = (c0, c1, c2), ctOut = (out0, out1)"""
        check(lib().lr_bfv_relinearize(self.h, ct[0].h, ct[1].h, ct[2].h, evakey.h, ctOut[0].h, ctOut[1].h))

    def BfvPermute(self, ct0, generator, switchKey, ctOut):
        """bfv.evaluator.permute (bfv/evaluator.go:711): the body of RotateRows (generator = galElRotRow) and of RotateColumns with
        the key of that rotation (galElRotColLeft[k]); ct0, ctOut: pairs of Poly over Q, coefficient domain; ctOut may be ct0"""
        check(lib().lr_bfv_rotate(self.h, ct0[0].h, ct0[1].h, C.c_uint64(int(generator)), switchKey.h, ctOut[0].h, ctOut[1].h))

    def BfvRotateColumnsPow2(self, ct0, generator, k, pow2_keys, ctOut):
        """bfv.evaluator.rotateColumnsPow2 (bfv/evaluator.go:636-662): rotation by k as the chain of the power-of-two rotations in
        its binary expansion; pow2_keys: {2^i: SwitchingKey image}; generator = GaloisGen (left) or its inverse mod 2N (right)"""
        mask = (self.contextQ.N << 1) - 1
        if ctOut[0] is not ct0[0]:
            self.contextQ.Copy(ct0[0], ctOut[0])                     # :647-648
            self.contextQ.Copy(ct0[1], ctOut[1])
        idx = 1
        while k > 0:
            if k & 1:
                self.BfvPermute(ctOut, generator, pow2_keys[idx], ctOut)   # :655
            generator = (generator * generator) & mask                     # :658-659
            idx <<= 1
            k >>= 1

    def BfvRelinearizeDeg(self, ct, evakeys, ctOut):
        """bfv.evaluator.Relinearize of a ciphertext of any degree len(ct) - 1 <= 5 as one call (lr_bfv_relinearize_deg,
        bfv/evaluator.go:480-499): evakeys[k] = the image of evakey.evakey[k], the key from s^(k + 2); ctOut may be (ct[0], ct[1])"""
        degree = len(ct) - 1
        if len(evakeys) < degree - 1:
            raise ValueError("one key per degree above 1")
        cts = (C.c_void_p * max(degree + 1, 1))(*[p.h.value if p is not None else None for p in ct])
        keys = (C.c_void_p * max(len(evakeys), 1))(*[k.h.value if k is not None else None for k in evakeys])
        check(lib().lr_bfv_relinearize_deg(self.h, cts, degree, keys if len(evakeys) else None, ctOut[0].h, ctOut[1].h))

    def BfvRotateChain(self, ct0, generators, switchKeys, accumulate, ctOut):
        """a chain of bfv.evaluator.permute steps as one call (lr_bfv_rotate_chain): step i rotates the running ciphertext by the Galois
        element generators[i] under switchKeys[i] and replaces it (accumulate False: rotateColumnsPow2, bfv/evaluator.go:637-666) or is
        added to it (True: InnerSum's loop, :701-707); ctOut may be ct0; no step copies"""
        n = len(generators)
        if len(switchKeys) != n:
            raise ValueError("one key per Galois element")
        g = (C.c_uint64 * max(n, 1))(*[int(x) for x in generators])
        keys = (C.c_void_p * max(n, 1))(*[k.h.value if k is not None else None for k in switchKeys])
        check(lib().lr_bfv_rotate_chain(self.h, ct0[0].h, ct0[1].h, n, g, keys, 1 if accumulate else 0, ctOut[0].h, ctOut[1].h))

    def BfvRotateColumnsPow2Chain(self, ct0, generator, k, pow2_keys, ctOut):
        """BfvRotateColumnsPow2 as ONE call: the set bits of k become the steps of a replace chain"""
        mask = (self.contextQ.N << 1) - 1
        gens, keys, idx = [], [], 1
        while k > 0:
            if k & 1:
                gens.append(generator)
                keys.append(pow2_keys[idx])
            generator = (generator * generator) & mask
            idx <<= 1
            k >>= 1
        self.BfvRotateChain(ct0, gens, keys, False, ctOut)

    def BfvInnerSum(self, ct0, col_keys, row_key, ctOut):
        """bfv.evaluator.InnerSum (bfv/evaluator.go:691-708) as one call (lr_bfv_inner_sum): col_keys[i] = the image of
        evakeyRotColLeft[2^i], i = 0 .. log2(N) - 2; row_key = the image of evakeyRotRow; ctOut may be ct0"""
        n = len(col_keys)
        keys = (C.c_void_p * max(n, 1))(*[k.h.value if k is not None else None for k in col_keys])
        check(lib().lr_bfv_inner_sum(self.h, ct0[0].h, ct0[1].h, n, keys, row_key.h if row_key is not None else None, ctOut[0].h, ctOut[1].h))

    def MulRelin(self, level, ct0, ct1, evakey, ctOut):
        """evaluator.MulRelin (ckks/evaluator.go:1016).  ct0, ct1: tuples of Poly -- (value[0], value[1]) for a ciphertext,
        (value[0],) for a plaintext; ctOut: pair, or triple when evakey is None and both operands are ciphertexts
        (degree-2 result, :1061-1066)."""
        if len(ct0) + len(ct1) == 3:                                     # plaintext x ciphertext, :1113-1131
            pt, ct = (ct0, ct1) if len(ct0) == 1 else (ct1, ct0)
            check(lib().lr_ckks_mul_plain(self.h, level, pt[0].h, ct[0].h, ct[1].h, ctOut[0].h, ctOut[1].h))
        elif evakey is None:
            check(lib().lr_ckks_mul_norelin(self.h, level, ct0[0].h, ct0[1].h, ct1[0].h, ct1[1].h,
                                            ctOut[0].h, ctOut[1].h, ctOut[2].h))
        else:
            check(lib().lr_ckks_mulrelin(self.h, level, ct0[0].h, ct0[1].h, ct1[0].h, ct1[1].h, evakey.h,
                                         ctOut[0].h, ctOut[1].h))

    def Rescale(self, ct):
        check(lib().lr_ckks_rescale(self.h, ct[0].h, ct[1].h))

    def EncryptPk(self, level, u, pk, e, plaintext, ctOut):
        """pkEncryptor.encrypt, the branch through the special primes (ckks/encryptor.go:205-234), after the sampling:
        u = SampleTernaryMontgomeryNTT over QP, e = the two Gaussian samples as residues over QP (coefficient domain,
        what SampleAndAdd adds, ring/gaussianSampler.go:254-274), pk = (pk0, pk1) over QP, plaintext over Q (NTT)."""
        check(lib().lr_ckks_encrypt_pk(self.h, level, u.h, pk[0].h, pk[1].h, e[0].h, e[1].h, plaintext.h, ctOut[0].h, ctOut[1].h))

    def Decrypt(self, level, ct, sk, ptOut):
        """decryptor.Decrypt (ckks/decryptor.go:53-78): Horner evaluation at the secret key (Montgomery NTT form)."""
        arr = (C.c_void_p * len(ct))(*[c.h.value for c in ct])
        check(lib().lr_ckks_decrypt(self.h, level, arr, len(ct) - 1, sk.h, ptOut.h))

    def PermuteNTT(self, level, ct0, gen, rotkey, ctOut):
        """evaluator.permuteNTT (ckks/evaluator.go:1448): RotateColumns with the key of that rotation, or Conjugate.
        gen: the Galois element whose PermuteNTTIndex the reference stores next to the key."""
        check(lib().lr_ckks_rotate(self.h, level, ct0[0].h, ct0[1].h, int(gen), rotkey.h, ctOut[0].h, ctOut[1].h))

    def RotateColumnsPow2(self, level, ct0, k, pow2_keys, ctOut):
        """evaluator.rotateColumnsPow2 (ckks/evaluator.go:1408-1430): rotation by k as the chain of the power-of-two
        rotations in its binary expansion.  pow2_keys: {2^i: (Galois element, SwitchingKey image)}."""
        if ctOut[0] is not ct0[0]:
            self.contextQ.CopyLvl(level, ct0[0], ctOut[0])     # :1417-1418
            self.contextQ.CopyLvl(level, ct0[1], ctOut[1])
        idx = 1
        while k > 0:
            if k & 1:
                gen, key = pow2_keys[idx]
                self.PermuteNTT(level, ctOut, gen, key, ctOut)  # :1424
            idx <<= 1
            k >>= 1

    def RotateChain(self, level, ct0, gens, keys, accumulate, ctOut):
        """a chain of evaluator.permuteNTT steps as one call (lr_ckks_rotate_chain): step i rotates the running ciphertext by the Galois
        element gens[i] under keys[i] and replaces it (accumulate False: rotateColumnsPow2, ckks/evaluator.go:1402-1424) or is added to
        it (True: the slot-sum loop RotateColumns; Add); ctOut may be ct0; no step copies"""
        n = len(gens)
        if len(keys) != n:
            raise ValueError("one key per Galois element")
        g = (C.c_uint64 * max(n, 1))(*[int(x) for x in gens])
        ks = (C.c_void_p * max(n, 1))(*[k.h.value if k is not None else None for k in keys])
        check(lib().lr_ckks_rotate_chain(self.h, level, ct0[0].h, ct0[1].h, n, g, ks, 1 if accumulate else 0, ctOut[0].h, ctOut[1].h))

    def RotateColumnsPow2Chain(self, level, ct0, k, pow2_keys, ctOut):
        """RotateColumnsPow2 as ONE call: the set bits of k become the steps of a replace chain"""
        gens, keys, idx = [], [], 1
        while k > 0:
            if k & 1:
                gen, key = pow2_keys[idx]
                gens.append(gen)
                keys.append(key)
            idx <<= 1
            k >>= 1
        self.RotateChain(level, ct0, gens, keys, False, ctOut)

    def PowerBasis(self, level, c1, schedule, evakey, outs):
        """The products of a power basis as one call (lr_ckks_power_basis): c1 = C[1] at `level`, schedule: a CkksBasisSchedule
        (ckks_power_basis_schedule), outs[k] = (out0, out1) receives C[schedule.products[k].n] on limbs 0 .. level_after.  The same bits
        as per product MulRelin, Rescale (n_rescales times) and the CkksCombine call of the Chebyshev tail."""
        n = len(schedule.products)
        if len(outs) != n:
            raise ValueError("one output per product")
        prods = (nat.BasisProduct * max(n, 1))(*schedule.products)
        if n == 0:      # an empty basis (targets [] or [1]): the call checks C[1] and the key and launches nothing
            mult = add = np.zeros((1, level + 1), dtype=np.uint64)
        else:
            mult = np.ascontiguousarray(schedule.mult, dtype=np.uint64).reshape(n, -1)
            add = np.ascontiguousarray(schedule.add, dtype=np.uint64).reshape(n, -1)
        if mult.shape != add.shape:
            raise LatticeRingError(3, "PowerBasis: mult and add have one shape")
        o0 = (C.c_void_p * max(n, 1))(*[o[0].h.value if o[0] is not None else None for o in outs])
        o1 = (C.c_void_p * max(n, 1))(*[o[1].h.value if o[1] is not None else None for o in outs])
        check(lib().lr_ckks_power_basis(self.h, n, prods, mult.ctypes.data_as(C.c_void_p), add.ctypes.data_as(C.c_void_p),
                                        mult.shape[1], level, c1[0].h, c1[1].h, evakey.h, o0, o1))
        return outs

    def RotateHoisted(self, level, ct0, gens, rotkeys, ctOuts):
        """evaluator.RotateHoisted (ckks/evaluator.go:1252): ctOuts[r] = rotation of ct0 by the Galois element gens[r]."""
        n = len(gens)
        g = (C.c_uint64 * n)(*[int(x) for x in gens])
        keys = (C.c_void_p * n)(*[k.h.value for k in rotkeys])
        o0 = (C.c_void_p * n)(*[o[0].h.value for o in ctOuts])
        o1 = (C.c_void_p * n)(*[o[1].h.value for o in ctOuts])
        check(lib().lr_ckks_rotate_hoisted(self.h, level, ct0[0].h, ct0[1].h, n, g, keys, o0, o1))


class CkksBatcher:
    """Merges the MulRelin calls of concurrent evaluators -- the reference's model is one evaluator per goroutine, one ciphertext
    per call (examples/dbfv/psi/psi.go:215-233) -- into batched launches (lr_ckks_batcher_* in include/lattigo_ring.h).
    One lane = one CkksPlan over its own pair of contexts on its own stream; the batcher builds them."""

    def __init__(self, N, Q, P, max_batch=64, lanes=2, device=0):
        self.lanes = []
        for i in range(lanes):
            cq, cp = Context(N, Q, device=device), Context(N, P, device=device)
            self.lanes.append((cq, cp, CkksPlan(cq, cp, max_batch)))
        arr = (C.c_void_p * lanes)(*[ln[2].h for ln in self.lanes])
        h = C.c_void_p()
        check(lib().lr_ckks_batcher_create(arr, lanes, C.byref(h)))
        self.h = h
        self.max_batch = max_batch

    def __del__(self):
        try:
            if getattr(self, "h", None):
                lib().lr_ckks_batcher_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def NewSwitchingKey(self):
        """the key image every calling evaluator passes (one handle: calls share a batch only over the same key)"""
        return self.lanes[0][2].NewSwitchingKey()

    def MulRelin(self, level, ct0, ct1, evakey, ctOut):
        """evaluator.MulRelin (ckks/evaluator.go:1016) of two ciphertexts with key; blocks until this call's result is complete.
        Call it from as many host threads as there are evaluators (ctypes releases the GIL for the call)."""
        check(lib().lr_ckks_batcher_mulrelin(self.h, level, ct0[0].h, ct0[1].h, ct1[0].h, ct1[1].h, evakey.h, ctOut[0].h, ctOut[1].h))

    def PermuteNTT(self, level, ct0, gen, rotkey, ctOut):
        """evaluator.permuteNTT (ckks/evaluator.go:1448) = RotateColumns with the key of that rotation / Conjugate; blocks until this
        call's result is complete; calls with the same (level, gen, key) in flight together share a launch"""
        check(lib().lr_ckks_batcher_rotate(self.h, level, ct0[0].h, ct0[1].h, C.c_uint64(int(gen)), rotkey.h, ctOut[0].h, ctOut[1].h))

    def Stats(self):
        b, p, l = C.c_uint64(), C.c_uint64(), C.c_int()
        check(lib().lr_ckks_batcher_stats(self.h, C.byref(b), C.byref(p), C.byref(l)))
        return {"batches": b.value, "products": p.value, "largest": l.value}


class BfvPlan:
    """What bfv.NewEvaluator builds around the ring for Mul (bfv/evaluator.go:89-112) and the tensorAndRescale
    call sequence (:278-464) for two degree-1 ciphertexts, device-resident."""

    def __init__(self, contextQ, contextQMul, t, max_batch=1, options=None):
        self.contextQ, self.contextQMul, self.t = contextQ, contextQMul, int(t)
        h = C.c_void_p()
        if options is None:
            check(lib().lr_bfv_plan_create(contextQ.h, contextQMul.h, self.t, max_batch, C.byref(h)))
        else:
            check(lib().lr_bfv_plan_create_ex(contextQ.h, contextQMul.h, self.t, max_batch, C.byref(options), C.byref(h)))
        self.h = h

    def __del__(self):
        try:
            if getattr(self, "h", None):
                lib().lr_bfv_plan_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def Mul(self, ct0, ct1, ctOut):
        """ct0, ct1: pairs of Poly over Q (coefficient domain); ctOut: triple (degree 2)."""
        check(lib().lr_bfv_mul(self.h, ct0[0].h, ct0[1].h, ct1[0].h, ct1[1].h, ctOut[0].h, ctOut[1].h, ctOut[2].h))

    def MulDeg(self, ct0, ct1, ctOut):
        """evaluator.Mul (bfv/evaluator.go:467) for operands of any degree with len(ct0) + len(ct1) <= 7 (lr_bfv_mul_deg): ct0, ct1
        sequences of Poly over Q (coefficient domain; a Plaintext is a sequence of one), ctOut of len(ct0) + len(ct1) - 1 distinct
        Poly.  The same Poly objects in ct0 and ct1 are the squaring case.  An output may be an operand."""
        if len(ctOut) != len(ct0) + len(ct1) - 1:
            raise LatticeRingError(4, "MulDeg: ctOut must hold len(ct0) + len(ct1) - 1 polys")      # LR_ERR_ARG
        arr = lambda ps: (C.c_void_p * max(len(ps), 1))(*[None if p is None else p.h.value for p in ps])
        check(lib().lr_bfv_mul_deg(self.h, arr(ct0), len(ct0) - 1, arr(ct1), len(ct1) - 1, arr(ctOut)))

    def NewRelinearizer(self, contextP, max_batch=1):
        """the key-switch half of bfv.NewEvaluator (decomposer, baseconverterQ1P, keyswitchpool: bfv/evaluator.go:100-112) over
        (contextQ, contextP): a CkksPlan, whose BfvRelinearize / BfvSwitchKeys / NewSwitchingKey serve Evaluator.Relinearize"""
        return CkksPlan(self.contextQ, contextP, max_batch)


class BfvEncoder:
    """bfv.Encoder (bfv/encoder.go:10-182) for a batch of plaintexts on the device (lr_bfv_encoder): what bfv.NewEncoder builds --
    contextT = (N, [t]), indexMatrix, deltaMont, the SimpleScaler, the one-limb pool -- for up to max_batch plaintexts per call.
    Slots are numpy arrays [batch, n] (or [n] for one plaintext); plaintexts are Poly over contextQ in the coefficient domain."""

    def __init__(self, contextQ, t, max_batch=1, options=None):
        self.contextQ, self.t, self.max_batch = contextQ, int(t), int(max_batch)
        h = C.c_void_p()
        if options is None:
            check(lib().lr_bfv_encoder_create(contextQ.h, self.t, max_batch, C.byref(h)))
        else:
            check(lib().lr_bfv_encoder_create_ex(contextQ.h, self.t, max_batch, C.byref(options), C.byref(h)))
        self.h = h

    def __del__(self):
        try:
            if getattr(self, "h", None):
                lib().lr_bfv_encoder_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def tables(self):
        """(indexMatrix[N], deltaMont[|Q|]) as computed on the host by NewEncoder / GenLiftParams"""
        index = np.zeros(self.contextQ.N, dtype=np.uint64)
        delta = np.zeros(len(self.contextQ.Modulus), dtype=np.uint64)
        check(lib().lr_bfv_encoder_tables(self.h, index.ctypes.data_as(nat.u64p), delta.ctypes.data_as(nat.u64p)))
        return index, delta

    def fused(self):
        """True when the handle runs the fused kernels, False on the composed route (lr_bfv_encoder_route)"""
        f = C.c_int(0)
        check(lib().lr_bfv_encoder_route(self.h, C.byref(f)))
        return bool(f.value)

    def NewPlaintext(self, batch=1):
        return self.contextQ.NewPoly(batch)

    def _encode(self, fn, dtype, coeffs, plaintext):
        a = np.ascontiguousarray(coeffs, dtype=dtype)
        if a.ndim == 1:
            a = a[None]
        if a.ndim != 2:
            raise LatticeRingError(3, "expected slots of shape [batch, n], got %s" % (a.shape,))      # LR_ERR_SHAPE
        check(fn(self.h, a.ctypes.data_as(C.c_void_p), a.shape[1], a.shape[0], plaintext.h))
        return plaintext

    def EncodeUint(self, coeffs, plaintext):  # bfv/encoder.go:71
        return self._encode(lib().lr_bfv_encode_uint, np.uint64, coeffs, plaintext)

    def EncodeInt(self, coeffs, plaintext):  # :95
        return self._encode(lib().lr_bfv_encode_int, np.int64, coeffs, plaintext)

    def _decode(self, fn, dtype, plaintext):
        out = np.empty((plaintext.batch, self.contextQ.N), dtype=dtype)
        check(fn(self.h, plaintext.h, plaintext.batch, out.ctypes.data_as(C.c_void_p)))
        return out

    def DecodeUint(self, plaintext):  # :140
        return self._decode(lib().lr_bfv_decode_uint, np.uint64, plaintext)

    def DecodeInt(self, plaintext):  # :158
        return self._decode(lib().lr_bfv_decode_int, np.int64, plaintext)

    def EncodeDevice(self, device_ptr, n_values, batch, signed, plaintext):
        """slots already on the device, [batch][n_values] uint64 / int64 (e.g. a torch tensor's data_ptr()); stream-ordered"""
        check(lib().lr_bfv_encode_device(self.h, C.c_void_p(device_ptr), n_values, batch, 1 if signed else 0, plaintext.h))
        return plaintext

    def DecodeDevice(self, plaintext, signed, device_ptr):
        """the slots to device memory of [batch][N] words; stream-ordered, no synchronisation"""
        check(lib().lr_bfv_decode_device(self.h, plaintext.h, plaintext.batch, 1 if signed else 0, C.c_void_p(device_ptr)))


def NewBfvEncoder(contextQ, t, max_batch=1, options=None):  # bfv.NewEncoder, bfv/encoder.go:28
    return BfvEncoder(contextQ, t, max_batch, options)


class _QpHandle:
    """What BfvEncryptor, CkksEncryptor, KeyGenerator, Collective and Refresh share (csrc/lr_qp_handle.hpp): a handle over contextQ and contextP
    with a max_batch, made by <_abi>_create / <_abi>_create_ex and freed by <_abi>_destroy, and the check of the compact randomness'
    size.  contextP None goes to the library as NULL: it says which handles and which calls need a P."""

    _abi = None

    def __init__(self, contextQ, contextP, max_batch=1, options=None):
        self.contextQ, self.contextP, self.max_batch = contextQ, contextP, int(max_batch)
        h = C.c_void_p()
        hP = None if contextP is None else contextP.h
        if options is None:
            check(getattr(lib(), self._abi + "_create")(contextQ.h, hP, max_batch, C.byref(h)))
        else:
            check(getattr(lib(), self._abi + "_create_ex")(contextQ.h, hP, max_batch, C.byref(options), C.byref(h)))
        self.h = h

    def __del__(self):
        try:
            if getattr(self, "h", None):
                getattr(lib(), self._abi + "_destroy")(self.h)
                self.h = None
        except Exception:
            pass

    def _bytes(self, a, batch, per_poly):
        a = np.ascontiguousarray(a, dtype=np.uint8)
        if a.size != batch * per_poly:
            raise LatticeRingError(3, "expected %d x %d bytes of randomness, got %s" % (batch, per_poly, a.shape))      # LR_ERR_SHAPE
        return a


class BfvEncryptor(_QpHandle):
    """bfv.Encryptor (bfv/encryptor.go:100-345) for a batch of ciphertexts on the device (lr_bfv_encryptor), after the sampling: the
    randomness arrives as the samplers' compact decisions.  u_bits = (coeff_bits, sign_bits), uint8 [batch, N / 8] each
    (ring/ternarySampler.go:157-177); e = uint8 [batch, N] per sampled poly, magnitude in the low 7 bits and sign in bit 7
    (ring/gaussianSampler.go:247).  Keys are Poly of contextQ over Q||P (fast: over Q) in NTT + Montgomery form, batch 1 or the
    call's; plaintext and ctOut are Poly over Q in the coefficient domain.  contextP None: only the fast forms."""

    _abi = "lr_bfv_encryptor"

    def EncryptPk(self, pk, u_bits, e, plaintext, ctOut, fast=False):  # pkEncryptor.encrypt, bfv/encryptor.go:169
        batch, N = ctOut[0].batch, self.contextQ.N
        uc, us = self._bytes(u_bits[0], batch, N // 8), self._bytes(u_bits[1], batch, N // 8)
        e0, e1 = self._bytes(e[0], batch, N), self._bytes(e[1], batch, N)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        check(lib().lr_bfv_encrypt_pk(self.h, 1 if fast else 0, pk[0].h, pk[1].h, p(uc), p(us), p(e0), p(e1), plaintext.h, batch,
                                      ctOut[0].h, ctOut[1].h))
        return ctOut

    def EncryptSk(self, sk, crp, e, plaintext, ctOut, fast=False):  # skEncryptor.encrypt, :306
        batch = ctOut[0].batch
        eb = self._bytes(e, batch, self.contextQ.N)
        check(lib().lr_bfv_encrypt_sk(self.h, 1 if fast else 0, sk.h, crp.h, eb.ctypes.data_as(C.c_void_p), plaintext.h, batch,
                                      ctOut[0].h, ctOut[1].h))
        return ctOut

    def EncryptPkDevice(self, pk, u_bits_ptrs, e_ptrs, plaintext, ctOut, fast=False):
        """the same with the randomness in device memory (pointers, e.g. a torch uint8 tensor's data_ptr()); stream-ordered"""
        v = C.c_void_p
        check(lib().lr_bfv_encrypt_pk_device(self.h, 1 if fast else 0, pk[0].h, pk[1].h, v(u_bits_ptrs[0]), v(u_bits_ptrs[1]), v(e_ptrs[0]),
                                             v(e_ptrs[1]), plaintext.h, ctOut[0].batch, ctOut[0].h, ctOut[1].h))
        return ctOut

    def EncryptSkDevice(self, sk, crp, e_ptr, plaintext, ctOut, fast=False):
        check(lib().lr_bfv_encrypt_sk_device(self.h, 1 if fast else 0, sk.h, crp.h, C.c_void_p(e_ptr), plaintext.h, ctOut[0].batch,
                                             ctOut[0].h, ctOut[1].h))
        return ctOut


class BfvDecryptor:
    """bfv.Decryptor (bfv/decryptor.go:28-75) for a batch of ciphertexts on the device (lr_bfv_decryptor)."""

    def __init__(self, contextQ, max_batch=1):
        self.contextQ, self.max_batch = contextQ, int(max_batch)
        h = C.c_void_p()
        check(lib().lr_bfv_decryptor_create(contextQ.h, max_batch, C.byref(h)))
        self.h = h

    def __del__(self):
        try:
            if getattr(self, "h", None):
                lib().lr_bfv_decryptor_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def Decrypt(self, ct, sk, ptOut):  # decryptor.Decrypt, bfv/decryptor.go:55; ct = the components, degree = len(ct) - 1
        arr = (C.c_void_p * max(len(ct), 1))(*[None if p is None else p.h.value for p in ct])
        check(lib().lr_bfv_decrypt(self.h, arr, len(ct) - 1, sk.h, ptOut.h, ptOut.batch))
        return ptOut


def NewBfvEncryptor(contextQ, contextP, max_batch=1, options=None):  # bfv.NewEncryptorFromPk / FromSk, bfv/encryptor.go:72-98
    return BfvEncryptor(contextQ, contextP, max_batch, options)


def NewBfvDecryptor(contextQ, max_batch=1):  # bfv.NewDecryptor, bfv/decryptor.go:28
    return BfvDecryptor(contextQ, max_batch)


class CkksEncoder:
    """ckks.Encoder (ckks/encoder.go:10-226) for a batch of plaintexts on the device (lr_ckks_encoder): rotGroup, the root table, the
    decoder's CRT tables and a pool for up to max_batch plaintexts per call.  roots = the reference's roots[0 .. m], m = 2 N, as a
    complex128 array of m + 1 entries (None: the library fills it with the host libm).  Slot values are complex128 arrays
    [batch, slots] (or [slots] for one plaintext); plaintexts are Poly over contextQ in the NTT domain."""

    def __init__(self, contextQ, max_batch=1, roots=None, options=None):
        self.contextQ, self.max_batch = contextQ, int(max_batch)
        rp = None
        if roots is not None:
            r = np.ascontiguousarray(roots, dtype=np.complex128)
            if r.shape != (2 * contextQ.N + 1,):
                raise LatticeRingError(3, "expected 2 N + 1 roots, got %s" % (r.shape,))                # LR_ERR_SHAPE
            rp = r.ctypes.data_as(C.c_void_p)
        h = C.c_void_p()
        if options is None:
            check(lib().lr_ckks_encoder_create(contextQ.h, max_batch, rp, C.byref(h)))
        else:
            check(lib().lr_ckks_encoder_create_ex(contextQ.h, max_batch, rp, C.byref(options), C.byref(h)))
        self.h = h

    def __del__(self):
        try:
            if getattr(self, "h", None):
                lib().lr_ckks_encoder_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def tables(self):
        """(rotGroup[m / 2], roots[m + 1] complex128) as NewEncoder holds them"""
        m = 2 * self.contextQ.N
        rot = np.zeros(m // 2, dtype=np.uint64)
        roots = np.zeros(m + 1, dtype=np.complex128)
        check(lib().lr_ckks_encoder_tables(self.h, rot.ctypes.data_as(nat.u64p), roots.ctypes.data_as(C.c_void_p)))
        return rot, roots

    def fused(self, slots):
        """True when a call with this slot count runs the fused kernels, False on the tiled route (lr_ckks_encoder_route)"""
        f = C.c_int(0)
        check(lib().lr_ckks_encoder_route(self.h, slots, C.byref(f)))
        return bool(f.value)

    def Encode(self, plaintext, values, level, scale):  # ckks/encoder.go:78; slots = values.shape[-1]
        a = np.ascontiguousarray(values, dtype=np.complex128)
        if a.ndim == 1:
            a = a[None]
        if a.ndim != 2:
            raise LatticeRingError(3, "expected slot values of shape [batch, slots], got %s" % (a.shape,))    # LR_ERR_SHAPE
        check(lib().lr_ckks_encode(self.h, a.ctypes.data_as(C.c_void_p), a.shape[1], level, float(scale), a.shape[0], plaintext.h))
        return plaintext

    def Decode(self, plaintext, slots, level, scale):  # :119
        out = np.empty((plaintext.batch, max(int(slots), 0)), dtype=np.complex128)
        check(lib().lr_ckks_decode(self.h, plaintext.h, slots, level, float(scale), plaintext.batch, out.ctypes.data_as(C.c_void_p)))
        return out

    def EncodeDevice(self, plaintext, device_ptr, slots, level, scale, batch):
        """slot values already on the device, [batch][slots] complex128 (e.g. a torch tensor's data_ptr()); stream-ordered"""
        check(lib().lr_ckks_encode_device(self.h, C.c_void_p(device_ptr), slots, level, float(scale), batch, plaintext.h))
        return plaintext

    def DecodeDevice(self, plaintext, slots, level, scale, device_ptr):
        """the slot values to device memory of [batch][slots] complex128; stream-ordered, no synchronisation"""
        check(lib().lr_ckks_decode_device(self.h, plaintext.h, slots, level, float(scale), plaintext.batch, C.c_void_p(device_ptr)))


def NewCkksEncoder(contextQ, max_batch=1, roots=None, options=None):  # ckks.NewEncoder, ckks/encoder.go:31
    return CkksEncoder(contextQ, max_batch, roots, options)


class CkksEncryptor(_QpHandle):
    """ckks.Encryptor (ckks/encryptor.go:100-362) for a batch of ciphertexts on the device (lr_ckks_encryptor), after the sampling.  The
    randomness is BfvEncryptor's compact form: u_bits = (coeff_bits, sign_bits), uint8 [batch, N / 8] each; e = uint8 [batch, N] per
    sampled poly, magnitude in the low 7 bits and sign in bit 7.  Keys are Poly of contextQ over Q||P (fast: over Q) in NTT + Montgomery
    form, batch 1 or the call's; plaintext and ctOut are Poly of contextQ in the NTT domain with at least level + 1 limbs (what
    CkksEncoder.Encode writes and CkksPlan.Decrypt reads); limbs above level are not touched.  contextP None: only the fast forms."""

    _abi = "lr_ckks_encryptor"

    def EncryptPk(self, pk, u_bits, e, plaintext, ctOut, level, fast=False):  # pkEncryptor.encrypt, ckks/encryptor.go:179
        batch, N = ctOut[0].batch, self.contextQ.N
        uc, us = self._bytes(u_bits[0], batch, N // 8), self._bytes(u_bits[1], batch, N // 8)
        e0, e1 = self._bytes(e[0], batch, N), self._bytes(e[1], batch, N)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        check(lib().lr_ckks_encryptor_encrypt_pk(self.h, 1 if fast else 0, level, pk[0].h, pk[1].h, p(uc), p(us), p(e0), p(e1), plaintext.h,
                                                 batch, ctOut[0].h, ctOut[1].h))
        return ctOut

    def EncryptSk(self, sk, crp, e, plaintext, ctOut, level, fast=False):  # skEncryptor.encrypt, :318
        batch = ctOut[0].batch
        eb = self._bytes(e, batch, self.contextQ.N)
        check(lib().lr_ckks_encryptor_encrypt_sk(self.h, 1 if fast else 0, level, sk.h, crp.h, eb.ctypes.data_as(C.c_void_p), plaintext.h,
                                                 batch, ctOut[0].h, ctOut[1].h))
        return ctOut

    def EncryptPkDevice(self, pk, u_bits_ptrs, e_ptrs, plaintext, ctOut, level, fast=False):
        """the same with the randomness in device memory (pointers, e.g. a torch uint8 tensor's data_ptr()); stream-ordered"""
        v = C.c_void_p
        check(lib().lr_ckks_encryptor_encrypt_pk_device(self.h, 1 if fast else 0, level, pk[0].h, pk[1].h, v(u_bits_ptrs[0]),
                                                        v(u_bits_ptrs[1]), v(e_ptrs[0]), v(e_ptrs[1]), plaintext.h, ctOut[0].batch,
                                                        ctOut[0].h, ctOut[1].h))
        return ctOut

    def EncryptSkDevice(self, sk, crp, e_ptr, plaintext, ctOut, level, fast=False):
        check(lib().lr_ckks_encryptor_encrypt_sk_device(self.h, 1 if fast else 0, level, sk.h, crp.h, C.c_void_p(e_ptr), plaintext.h,
                                                        ctOut[0].batch, ctOut[0].h, ctOut[1].h))
        return ctOut


def NewCkksEncryptor(contextQ, contextP, max_batch=1, options=None):  # ckks.NewEncryptorFromPk / FromSk, ckks/encryptor.go:76-98
    return CkksEncryptor(contextQ, contextP, max_batch, options)


class KeyGenerator(_QpHandle):
    """ckks.KeyGenerator / bfv.KeyGenerator (ckks/keygen.go:79-494, bfv/keygen.go:70-441) on the device (lr_keygen), after the sampling.
    The randomness is the encryptors' compact form: bits = (coeff_bits, sign_bits), uint8 [batch, N / 8] each; e = uint8 [..., N] per
    sampled poly, magnitude in the low 7 bits and sign in bit 7.  Every key is a Poly of contextQ over Q||P in NTT + Montgomery form; a
    switching key is the image CkksPlan.NewSwitchingKey allocates, whose odd members hold the caller's uniform polys on entry and are not
    written.  contextP None: only the secret key and the public key, over Q."""

    _abi = "lr_keygen"

    @property
    def beta(self):
        if self.contextP is None:
            raise LatticeRingError(4, "key generator: modulus P is empty (ckks/keygen.go:249-251)")      # LR_ERR_ARG, as the C calls refuse
        nQ, nP = len(self.contextQ.Modulus), len(self.contextP.Modulus)
        return -(-nQ // nP)

    def NewKey(self, batch=1):
        """storage for a secret key or one half of a public key: `batch` polys over Q||P"""
        return Poly(self.contextQ, len(self.contextQ.Modulus) + (len(self.contextP.Modulus) if self.contextP else 0), batch)

    def NewSwitchingKey(self):
        """storage for SwitchingKey.evakey (ckks/keygen.go:68-70): beta x 2 polys over Q||P"""
        beta = self.beta
        return Poly(self.contextQ, len(self.contextQ.Modulus) + len(self.contextP.Modulus), 2 * beta)

    @staticmethod
    def _keys(evks):
        return (C.c_void_p * len(evks))(*[k.h.value for k in evks])

    def GenSecretKey(self, bits, skOut):  # ckks/keygen.go:97
        batch, N = skOut.batch, self.contextQ.N
        c, s = self._bytes(bits[0], batch, N // 8), self._bytes(bits[1], batch, N // 8)
        check(lib().lr_keygen_secret_key(self.h, c.ctypes.data_as(C.c_void_p), s.ctypes.data_as(C.c_void_p), batch, skOut.h))
        return skOut

    def GenPublicKey(self, sk, e, pk):  # :138; pk = (pk0 out, pk1 = the uniform poly)
        batch = pk[0].batch
        eb = self._bytes(e, batch, self.contextQ.N)
        check(lib().lr_keygen_public_key(self.h, sk.h, eb.ctypes.data_as(C.c_void_p), batch, pk[0].h, pk[1].h))
        return pk

    def GenSwitchingKeys(self, skIn, skOut, e, evks):  # :247, one key per entry of evks
        eb = self._bytes(e, len(evks) * self.beta, self.contextQ.N)
        check(lib().lr_keygen_switching_keys(self.h, skIn.h, skOut.h, eb.ctypes.data_as(C.c_void_p), len(evks), self._keys(evks)))
        return evks

    def GenRelinKeys(self, sk, e, evks):  # ckks/keygen.go:192 (one key), bfv/keygen.go:172 (maxDegree keys)
        eb = self._bytes(e, len(evks) * self.beta, self.contextQ.N)
        check(lib().lr_keygen_relin_keys(self.h, sk.h, len(evks), eb.ctypes.data_as(C.c_void_p), self._keys(evks)))
        return evks

    def GenRotationKeys(self, sk, galois_elements, e, evks):  # genrotKey, :487, for each Galois element
        eb = self._bytes(e, len(evks) * self.beta, self.contextQ.N)
        if len(galois_elements) != len(evks):
            raise LatticeRingError(3, "one switching key per Galois element")
        check(lib().lr_keygen_rotation_keys(self.h, sk.h, _u64(galois_elements), len(evks), eb.ctypes.data_as(C.c_void_p), self._keys(evks)))
        return evks

    def Pow2GaloisElements(self):
        """the Galois elements of GenRotationKeysPow2 (:391-417) in its order: for n = 1, 2, .. < N / 2 the left rotation 5^n and the right
        rotation 5^(N / 2 - n), then the conjugation 2 N - 1 -- 2 (logN - 1) + 1 elements"""
        N = self.contextQ.N
        left = GenGaloisParams(N, 5)
        right = GenGaloisParams(N, pow(5, -1, 2 * N))
        out, n = [], 1
        while n < N >> 1:
            out += [left[n], right[n]]
            n <<= 1
        return out + [2 * N - 1]

    def GenRotationKeysPow2(self, sk, sampler_bytes, uniform):
        """GenRotationKeysPow2: returns {"left": {n: (element, key)}, "right": {n: (element, key)}, "conjugate": (element, key)}.
        sampler_bytes = uint8 [2 (logN - 1) + 1, beta, N]; uniform = uint64 [2 (logN - 1) + 1, beta, |Q| + |P|, N], the evakey[i][1] of
        every key in the order of Pow2GaloisElements (what NewUniformPoly drew: a key without them reveals the secret)."""
        gens = self.Pow2GaloisElements()
        rows, beta = len(self.contextQ.Modulus) + len(self.contextP.Modulus), self.beta
        uniform = np.asarray(uniform, dtype=np.uint64)
        if uniform.shape != (len(gens), beta, rows, self.contextQ.N):
            raise LatticeRingError(3, "expected uniform polys of shape %s, got %s" % ((len(gens), beta, rows, self.contextQ.N), uniform.shape))
        evks = []
        for a in uniform:
            img = np.zeros((2 * beta, rows, self.contextQ.N), dtype=np.uint64)
            img[1::2] = a
            evks.append(self.NewSwitchingKey().set(img))
        self.GenRotationKeys(sk, gens, sampler_bytes, evks)
        out = {"left": {}, "right": {}, "conjugate": (gens[-1], evks[-1])}
        for i in range(len(gens) // 2):
            out["left"][1 << i] = (gens[2 * i], evks[2 * i])
            out["right"][1 << i] = (gens[2 * i + 1], evks[2 * i + 1])
        return out

    # the same with the randomness in device memory (pointers, e.g. a torch uint8 tensor's data_ptr()); stream-ordered
    def GenSecretKeyDevice(self, bits_ptrs, skOut):
        check(lib().lr_keygen_secret_key_device(self.h, C.c_void_p(bits_ptrs[0]), C.c_void_p(bits_ptrs[1]), skOut.batch, skOut.h))
        return skOut

    def GenPublicKeyDevice(self, sk, e_ptr, pk):
        check(lib().lr_keygen_public_key_device(self.h, sk.h, C.c_void_p(e_ptr), pk[0].batch, pk[0].h, pk[1].h))
        return pk

    def GenSwitchingKeysDevice(self, skIn, skOut, e_ptr, evks):
        check(lib().lr_keygen_switching_keys_device(self.h, skIn.h, skOut.h, C.c_void_p(e_ptr), len(evks), self._keys(evks)))
        return evks

    def GenRelinKeysDevice(self, sk, e_ptr, evks):
        check(lib().lr_keygen_relin_keys_device(self.h, sk.h, len(evks), C.c_void_p(e_ptr), self._keys(evks)))
        return evks

    def GenRotationKeysDevice(self, sk, galois_elements, e_ptr, evks):
        check(lib().lr_keygen_rotation_keys_device(self.h, sk.h, _u64(galois_elements), len(evks), C.c_void_p(e_ptr), self._keys(evks)))
        return evks


def NewKeyGenerator(contextQ, contextP, max_batch=1, options=None):  # ckks.NewKeyGenerator, ckks/keygen.go:79
    return KeyGenerator(contextQ, contextP, max_batch, options)


class Collective(_QpHandle):
    """CKSProtocol and PCKSProtocol of dckks and dbfv (dckks/keyswitching.go, dckks/public_keyswitching.go and their dbfv twins) for a
    batch of ciphertexts on the device (lr_collective), after the sampling.  The randomness is the encryptors' compact form: e = uint8
    [batch, N] per sampled poly, magnitude in the low 7 bits and sign in bit 7 (the smudging sampler and the regular one differ only in the
    bytes drawn); u_bits = (coeff_bits, sign_bits), uint8 [batch, N / 8] each.  Keys are Poly of contextQ over Q||P in NTT + Montgomery
    form (the secret keys are read on the rows of Q), batch 1 or the call's.  CKKS c1 and shares: NTT domain, at least level + 1 limbs;
    BFV c1 and shares: coefficient domain over Q.  The batch of a call is that of its output."""

    _abi = "lr_collective"

    def _pcks_bytes(self, u_bits, e, batch):
        N = self.contextQ.N
        arrays = [self._bytes(u_bits[0], batch, N // 8), self._bytes(u_bits[1], batch, N // 8), self._bytes(e[0], batch, N),
                  self._bytes(e[1], batch, N)]
        return arrays, [a.ctypes.data_as(C.c_void_p) for a in arrays]

    def CkksCksShare(self, skInput, skOutput, c1, e, shareOut, level):  # CKSProtocol.GenShare, dckks/keyswitching.go:62
        eb = self._bytes(e, shareOut.batch, self.contextQ.N)
        check(lib().lr_collective_ckks_cks_share(self.h, level, skInput.h, skOutput.h, c1.h, eb.ctypes.data_as(C.c_void_p), shareOut.batch,
                                                 shareOut.h))
        return shareOut

    def BfvCksShare(self, skInput, skOutput, c1, e, shareOut):  # dbfv/keyswitching.go:74
        eb = self._bytes(e, shareOut.batch, self.contextQ.N)
        check(lib().lr_collective_bfv_cks_share(self.h, skInput.h, skOutput.h, c1.h, eb.ctypes.data_as(C.c_void_p), shareOut.batch, shareOut.h))
        return shareOut

    def CkksPcksShare(self, sk, pk, c1, u_bits, e, shareOut, level):  # PCKSProtocol.GenShare, dckks/public_keyswitching.go:63
        batch = shareOut[0].batch
        keep, p = self._pcks_bytes(u_bits, e, batch)
        check(lib().lr_collective_ckks_pcks_share(self.h, level, sk.h, pk[0].h, pk[1].h, c1.h, p[0], p[1], p[2], p[3], batch, shareOut[0].h,
                                                  shareOut[1].h))
        return shareOut

    def BfvPcksShare(self, sk, pk, c1, u_bits, e, shareOut):  # dbfv/public_keyswitching.go:111
        batch = shareOut[0].batch
        keep, p = self._pcks_bytes(u_bits, e, batch)
        check(lib().lr_collective_bfv_pcks_share(self.h, sk.h, pk[0].h, pk[1].h, c1.h, p[0], p[1], p[2], p[3], batch, shareOut[0].h,
                                                 shareOut[1].h))
        return shareOut

    def Aggregate(self, shares, out, level, base=None):
        """AggregateShares over all the parties' shares in their order and, with base = ct[0], KeySwitch's Add; one share and no base is
        KeySwitch's Copy.  out may be base or one of the shares."""
        hs = (C.c_void_p * len(shares))(*[s.h.value for s in shares])
        check(lib().lr_collective_aggregate(self.h, level, None if base is None else base.h, hs, len(shares), out.h))
        return out

    # the same with the randomness in device memory (pointers, e.g. a torch uint8 tensor's data_ptr()); stream-ordered
    def CkksCksShareDevice(self, skInput, skOutput, c1, e_ptr, shareOut, level):
        check(lib().lr_collective_ckks_cks_share_device(self.h, level, skInput.h, skOutput.h, c1.h, C.c_void_p(e_ptr), shareOut.batch, shareOut.h))
        return shareOut

    def BfvCksShareDevice(self, skInput, skOutput, c1, e_ptr, shareOut):
        check(lib().lr_collective_bfv_cks_share_device(self.h, skInput.h, skOutput.h, c1.h, C.c_void_p(e_ptr), shareOut.batch, shareOut.h))
        return shareOut

    def CkksPcksShareDevice(self, sk, pk, c1, u_bits_ptrs, e_ptrs, shareOut, level):
        v = C.c_void_p
        check(lib().lr_collective_ckks_pcks_share_device(self.h, level, sk.h, pk[0].h, pk[1].h, c1.h, v(u_bits_ptrs[0]), v(u_bits_ptrs[1]),
                                                         v(e_ptrs[0]), v(e_ptrs[1]), shareOut[0].batch, shareOut[0].h, shareOut[1].h))
        return shareOut

    def BfvPcksShareDevice(self, sk, pk, c1, u_bits_ptrs, e_ptrs, shareOut):
        v = C.c_void_p
        check(lib().lr_collective_bfv_pcks_share_device(self.h, sk.h, pk[0].h, pk[1].h, c1.h, v(u_bits_ptrs[0]), v(u_bits_ptrs[1]),
                                                        v(e_ptrs[0]), v(e_ptrs[1]), shareOut[0].batch, shareOut[0].h, shareOut[1].h))
        return shareOut


def NewCollective(contextQ, contextP, max_batch=1, options=None):  # NewCKSProtocol / NewPCKSProtocol of dckks and dbfv
    return Collective(contextQ, contextP, max_batch, options)


class Refresh(_QpHandle):
    """RefreshProtocol of dckks and dbfv (dckks/public_refresh.go, dbfv/public_refresh.go) for a batch of ciphertexts on the device
    (lr_refresh), after the sampling.  e = (e0, e1), uint8 [batch, N] each, the encryptors' bytes.  CKKS mask: uint64 [batch, W, N] word
    planes of signed integers, W = MaskWords(levelStart) (sampling.mask_word_planes packs Python integers); BFV mask: uint64 [batch, N]
    below t.  sk: Poly of contextQ in NTT + Montgomery form, batch 1 or the call's, over Q (CKKS) or Q||P (BFV).  CKKS polys are in the NTT
    domain, BFV polys in the coefficient domain (crs over Q||P).  contextP None or t = 0: the CKKS entry points only.  The batch of a call
    is that of its output."""

    _abi = "lr_refresh"

    def __init__(self, contextQ, contextP=None, t=0, max_batch=1, options=None):
        self.contextQ, self.contextP, self.t, self.max_batch = contextQ, contextP, int(t), int(max_batch)
        h = C.c_void_p()
        hP = None if contextP is None else contextP.h
        if options is None:
            check(lib().lr_refresh_create(contextQ.h, hP, self.t, max_batch, C.byref(h)))
        else:
            check(lib().lr_refresh_create_ex(contextQ.h, hP, self.t, max_batch, C.byref(options), C.byref(h)))
        self.h = h

    def MaskWords(self, levelStart):
        w = C.c_int()
        check(lib().lr_refresh_mask_words(self.h, levelStart, C.byref(w)))
        return w.value

    def _random(self, mask, e, batch, mask_words):
        N = self.contextQ.N
        m = np.ascontiguousarray(mask, dtype=np.uint64)
        if m.size != batch * mask_words * N:
            raise LatticeRingError(3, "expected %d x %d x %d mask words, got %s" % (batch, mask_words, N, m.shape))      # LR_ERR_SHAPE
        arrays = [m, self._bytes(e[0], batch, N), self._bytes(e[1], batch, N)]
        return arrays, [a.ctypes.data_as(C.c_void_p) for a in arrays]

    def CkksGenShares(self, sk, levelStart, c1, crs, mask, e, shares):  # dckks/public_refresh.go:43; shares = (shareDecrypt, shareRecrypt)
        batch = shares[0].batch
        keep, p = self._random(mask, e, batch, self.MaskWords(levelStart))
        check(lib().lr_refresh_ckks_shares(self.h, levelStart, sk.h, c1.h, crs.h, p[0], p[1], p[2], batch, shares[0].h, shares[1].h))
        return shares

    def CkksRecode(self, levelStart, polIn, polOut):  # :108
        check(lib().lr_refresh_ckks_recode(self.h, levelStart, polIn.h, polOut.h))
        return polOut

    def CkksFinalize(self, levelStart, c0, shares, out0):  # Decrypt :103, Recode :108, Recrypt :142
        check(lib().lr_refresh_ckks_finalize(self.h, levelStart, c0.h, shares[0].h, shares[1].h, out0.h))
        return out0

    def BfvGenShares(self, sk, c1, crs, mask, e, shares):  # dbfv/public_refresh.go:105
        batch = shares[0].batch
        keep, p = self._random(mask, e, batch, 1)
        check(lib().lr_refresh_bfv_shares(self.h, sk.h, c1.h, crs.h, p[0], p[1], p[2], batch, shares[0].h, shares[1].h))
        return shares

    def BfvFinalize(self, c0, crs, shares, ctOut):  # :193; ctOut = (out0, out1)
        check(lib().lr_refresh_bfv_finalize(self.h, c0.h, crs.h, shares[0].h, shares[1].h, ctOut[0].h, ctOut[1].h))
        return ctOut

    def Aggregate(self, shares, out, level):
        """Aggregate over all the parties' shares in their order; out may be one of the shares"""
        hs = (C.c_void_p * len(shares))(*[s.h.value for s in shares])
        check(lib().lr_refresh_aggregate(self.h, level, hs, len(shares), out.h))
        return out

    # the same with the randomness in device memory (pointers); stream-ordered
    def CkksGenSharesDevice(self, sk, levelStart, c1, crs, mask_ptr, e_ptrs, shares):
        v = C.c_void_p
        check(lib().lr_refresh_ckks_shares_device(self.h, levelStart, sk.h, c1.h, crs.h, v(mask_ptr), v(e_ptrs[0]), v(e_ptrs[1]),
                                                  shares[0].batch, shares[0].h, shares[1].h))
        return shares

    def BfvGenSharesDevice(self, sk, c1, crs, mask_ptr, e_ptrs, shares):
        v = C.c_void_p
        check(lib().lr_refresh_bfv_shares_device(self.h, sk.h, c1.h, crs.h, v(mask_ptr), v(e_ptrs[0]), v(e_ptrs[1]), shares[0].batch,
                                                 shares[0].h, shares[1].h))
        return shares


def NewRefresh(contextQ, contextP=None, t=0, max_batch=1, options=None):  # NewRefreshProtocol of dckks and dbfv
    return Refresh(contextQ, contextP, t, max_batch, options)


class Setup(_QpHandle):
    """The collective key setup of dckks and dbfv on the device (lr_setup), after the sampling: CKGProtocol, RKGProtocol (three rounds),
    RKGProtocolNaive (two rounds) and RTGProtocol (dbfv/publickey_gen.go, relinkey_gen.go, relinkey_gen_naive.go, rotkey_gen.go and their
    dckks twins) for n parties per call.  Every Poly is one of contextQ over Q||P in the NTT domain; sk, u and pk are in Montgomery form,
    crs and crp are not.  A share of beta polys is a Poly of batch beta, a share of beta pairs one of batch 2 beta (member 2 i = [i][0],
    2 i + 1 = [i][1]): the image CkksPlan.NewSwitchingKey allocates, so RkgKey, RkgNaiveKey and RtgKey write keys the key switch reads.
    e = uint8 [..., N] per sampled poly (magnitude in the low 7 bits, sign in bit 7), bits = (coeff_bits, sign_bits), uint8 [..., N / 8]
    each.  n is the number of output shares; sk and u have batch n or 1.  contextP None: only CkgShare and Aggregate, over Q."""

    _abi = "lr_setup"
    BFV, CKKS = 0, 1

    @property
    def beta(self):
        if self.contextP is None:
            raise LatticeRingError(4, "collective setup: modulus P is empty: only CKG and its aggregation work over Q")      # LR_ERR_ARG
        return -(-len(self.contextQ.Modulus) // len(self.contextP.Modulus))

    @property
    def rows(self):
        return len(self.contextQ.Modulus) + (len(self.contextP.Modulus) if self.contextP else 0)

    def NewPoly(self, batch=1):
        """`batch` polys over Q||P: a key, a CKG share, crs"""
        return Poly(self.contextQ, self.rows, batch)

    def NewShare(self):
        """a share of beta polys: RKG rounds one and three, an RTG share, crp"""
        return Poly(self.contextQ, self.rows, self.beta)

    def NewPairShare(self):
        """a share of beta pairs: RKG round two, both naive rounds, and every finished key"""
        return Poly(self.contextQ, self.rows, 2 * self.beta)

    @staticmethod
    def _ptrs(polys):
        return (C.c_void_p * len(polys))(*[p.h.value for p in polys])

    def CkgShare(self, sk, crs, e, shareOut):  # CKGProtocol.GenShare, dbfv/publickey_gen.go:54
        eb = self._bytes(e, shareOut.batch, self.contextQ.N)
        check(lib().lr_setup_ckg_share(self.h, sk.h, crs.h, eb.ctypes.data_as(C.c_void_p), shareOut.batch, shareOut.h))
        return shareOut

    def RkgRound1(self, u, sk, crp, e, shares):  # GenShareRoundOne, dbfv/relinkey_gen.go:215
        eb = self._bytes(e, len(shares) * self.beta, self.contextQ.N)
        check(lib().lr_setup_rkg_round1(self.h, u.h, sk.h, crp.h, eb.ctypes.data_as(C.c_void_p), len(shares), self._ptrs(shares)))
        return shares

    def RkgRound2(self, round1, sk, crp, e, shares):  # GenShareRoundTwo, :277; e = [n, beta, 2, N]
        eb = self._bytes(e, len(shares) * self.beta * 2, self.contextQ.N)
        check(lib().lr_setup_rkg_round2(self.h, round1.h, sk.h, crp.h, eb.ctypes.data_as(C.c_void_p), len(shares), self._ptrs(shares)))
        return shares

    def RkgRound3(self, round2, u, sk, e, shares):  # GenShareRoundThree, :322
        eb = self._bytes(e, len(shares) * self.beta, self.contextQ.N)
        check(lib().lr_setup_rkg_round3(self.h, round2.h, u.h, sk.h, eb.ctypes.data_as(C.c_void_p), len(shares), self._ptrs(shares)))
        return shares

    def RkgKey(self, round2, round3, evkOut):  # GenRelinearizationKey, :343; evkOut may be round2
        check(lib().lr_setup_rkg_key(self.h, round2.h, round3.h, evkOut.h))
        return evkOut

    def RkgNaiveRound1(self, scheme, sk, pk, e, u_bits, shares):  # dbfv/relinkey_gen_naive.go:59, dckks/relinkey_gen_naive.go:59
        n, N = len(shares), self.contextQ.N
        eb, c, s = self._bytes(e, n * self.beta * 2, N), self._bytes(u_bits[0], n * self.beta, N // 8), self._bytes(u_bits[1], n * self.beta, N // 8)
        v = lambda a: a.ctypes.data_as(C.c_void_p)
        check(lib().lr_setup_rkg_naive_round1(self.h, scheme, sk.h, pk[0].h, pk[1].h, v(eb), v(c), v(s), n, self._ptrs(shares)))
        return shares

    def RkgNaiveRound2(self, round1, sk, pk, v_bits, e, shares):  # :135
        n, N = len(shares), self.contextQ.N
        eb, c, s = self._bytes(e, n * self.beta * 2, N), self._bytes(v_bits[0], n * self.beta, N // 8), self._bytes(v_bits[1], n * self.beta, N // 8)
        v = lambda a: a.ctypes.data_as(C.c_void_p)
        check(lib().lr_setup_rkg_naive_round2(self.h, round1.h, sk.h, pk[0].h, pk[1].h, v(c), v(s), v(eb), n, self._ptrs(shares)))
        return shares

    def RkgNaiveKey(self, round2, evkOut):  # :187; evkOut may be round2
        check(lib().lr_setup_rkg_naive_key(self.h, round2.h, evkOut.h))
        return evkOut

    def RtgShare(self, sk, galois_elements, crp, e, shares):  # RTGProtocol.genShare, dbfv/rotkey_gen.go:139, for each Galois element
        if len(galois_elements) != len(shares):
            raise LatticeRingError(3, "one share per Galois element")
        eb = self._bytes(e, len(shares) * self.beta, self.contextQ.N)
        check(lib().lr_setup_rtg_share(self.h, sk.h, _u64(galois_elements), len(shares), crp.h, eb.ctypes.data_as(C.c_void_p), self._ptrs(shares)))
        return shares

    def RtgKey(self, share, crp, rotKeyOut):  # Finalize, :205
        check(lib().lr_setup_rtg_key(self.h, share.h, crp.h, rotKeyOut.h))
        return rotKeyOut

    def Aggregate(self, shares, out):
        """every Aggregate* of the four protocols over all the parties' shares in their order, over all of Q||P; out may be a share"""
        check(lib().lr_setup_aggregate(self.h, self._ptrs(shares), len(shares), out.h))
        return out

    # the same with the randomness in device memory (pointers, e.g. a torch uint8 tensor's data_ptr()); stream-ordered
    def CkgShareDevice(self, sk, crs, e_ptr, shareOut):
        check(lib().lr_setup_ckg_share_device(self.h, sk.h, crs.h, C.c_void_p(e_ptr), shareOut.batch, shareOut.h))
        return shareOut

    def RkgRound1Device(self, u, sk, crp, e_ptr, shares):
        check(lib().lr_setup_rkg_round1_device(self.h, u.h, sk.h, crp.h, C.c_void_p(e_ptr), len(shares), self._ptrs(shares)))
        return shares

    def RkgRound2Device(self, round1, sk, crp, e_ptr, shares):
        check(lib().lr_setup_rkg_round2_device(self.h, round1.h, sk.h, crp.h, C.c_void_p(e_ptr), len(shares), self._ptrs(shares)))
        return shares

    def RkgRound3Device(self, round2, u, sk, e_ptr, shares):
        check(lib().lr_setup_rkg_round3_device(self.h, round2.h, u.h, sk.h, C.c_void_p(e_ptr), len(shares), self._ptrs(shares)))
        return shares

    def RkgNaiveRound1Device(self, scheme, sk, pk, e_ptr, u_bits_ptrs, shares):
        v = C.c_void_p
        check(lib().lr_setup_rkg_naive_round1_device(self.h, scheme, sk.h, pk[0].h, pk[1].h, v(e_ptr), v(u_bits_ptrs[0]), v(u_bits_ptrs[1]),
                                                     len(shares), self._ptrs(shares)))
        return shares

    def RkgNaiveRound2Device(self, round1, sk, pk, v_bits_ptrs, e_ptr, shares):
        v = C.c_void_p
        check(lib().lr_setup_rkg_naive_round2_device(self.h, round1.h, sk.h, pk[0].h, pk[1].h, v(v_bits_ptrs[0]), v(v_bits_ptrs[1]), v(e_ptr),
                                                     len(shares), self._ptrs(shares)))
        return shares

    def RtgShareDevice(self, sk, galois_elements, crp, e_ptr, shares):
        check(lib().lr_setup_rtg_share_device(self.h, sk.h, _u64(galois_elements), len(shares), crp.h, C.c_void_p(e_ptr), self._ptrs(shares)))
        return shares


def NewSetup(contextQ, contextP, max_batch=1, options=None):  # NewCKGProtocol / NewEkgProtocol / NewEkgProtocolNaive / NewRotKGProtocol
    return Setup(contextQ, contextP, max_batch, options)


class BfvBatcher:
    """Merges the Mul and Relinearize calls of concurrent BFV evaluators -- the reference's own pooled workload: every task of
    examples/dbfv/psi/psi.go:215-233 calls evaluator.Mul and evaluator.Relinearize on one ciphertext pair -- into batched launches
    (lr_bfv_batcher_* in include/lattigo_ring.h).  One lane = a BfvPlan over (contextQ, contextQMul) and the key-switch plan over
    (contextQ, contextP) on their own stream; the batcher builds them."""

    def __init__(self, N, Q, P, QMul, t, max_batch=64, lanes=2, device=0):
        self.lanes = []
        for i in range(lanes):
            cq, cp, cm = Context(N, Q, device=device), Context(N, P, device=device), Context(N, QMul, device=device)
            self.lanes.append((cq, cp, cm, BfvPlan(cq, cm, t, max_batch), CkksPlan(cq, cp, max_batch)))
        muls = (C.c_void_p * lanes)(*[ln[3].h for ln in self.lanes])
        kss = (C.c_void_p * lanes)(*[ln[4].h for ln in self.lanes])
        h = C.c_void_p()
        check(lib().lr_bfv_batcher_create(muls, kss, lanes, C.byref(h)))
        self.h = h
        self.max_batch = max_batch

    def __del__(self):
        try:
            if getattr(self, "h", None):
                lib().lr_bfv_batcher_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def NewSwitchingKey(self):
        """the relinearisation key image every calling evaluator passes (one handle: calls share a batch only over the same key)"""
        return self.lanes[0][4].NewSwitchingKey()

    def Mul(self, ct0, ct1, ctOut):
        """evaluator.Mul (bfv/evaluator.go:467) of two degree-1 ciphertexts -> degree 2; blocks until this call's result is complete"""
        check(lib().lr_bfv_batcher_mul(self.h, ct0[0].h, ct0[1].h, ct1[0].h, ct1[1].h, ctOut[0].h, ctOut[1].h, ctOut[2].h))

    def Relinearize(self, ct, evakey, ctOut):
        """evaluator.Relinearize (bfv/evaluator.go:512) of a degree-2 ciphertext"""
        check(lib().lr_bfv_batcher_relinearize(self.h, ct[0].h, ct[1].h, ct[2].h, evakey.h, ctOut[0].h, ctOut[1].h))

    def Stats(self):
        b, p, l = C.c_uint64(), C.c_uint64(), C.c_int()
        check(lib().lr_bfv_batcher_stats(self.h, C.byref(b), C.byref(p), C.byref(l)))
        return {"batches": b.value, "products": p.value, "largest": l.value}
