package ring

// #include <stdlib.h>
// #include "lattigo_ring.h"
import "C"

import (
	"math/big"
	"runtime"
	"unsafe"
)

// Refresh: what NewRefreshProtocol of dckks and dbfv build (dckks/public_refresh.go:23-35, dbfv/public_refresh.go:79-96) -- tmp, tmp1,
// tmp2, hP, the basis extender -- with GenShares, Aggregate, Decrypt, Recode and Recrypt on the device, after the sampling.  The noise is
// the samplers' decisions in the compact form of BfvEncryptor (KYSampler.SampleCompact in bfv_encryptor.go), N bytes per sampled poly.
// The CKKS mask is what RandInt gives, centred (dckks/public_refresh.go:57-63), as two's-complement word planes (MaskWordPlanes); the
// BFV mask is contextT.NewUniformPoly's row.  A Go Poly is one polynomial, so the slice forms make one pair of shares per call; the
// Device forms take maxBatch ciphertexts' randomness in device memory.  contextP nil or t = 0: the CKKS methods only.
// One deviation from upstream: dbfv's rfp.hP is never zeroed, so a second GenShares on one RefreshProtocol accumulates unreduced noise;
// every call here behaves as the first call on a fresh RefreshProtocol.
type Refresh struct {
	contextQ, contextP *Context
	T                  uint64
	MaxBatch           int
	h                  *C.lr_refresh
}

func NewRefresh(contextQ, contextP *Context, t uint64, maxBatch int) *Refresh {
	r := &Refresh{contextQ: contextQ, contextP: contextP, T: t, MaxBatch: maxBatch}
	var hP *C.lr_context
	if contextP != nil {
		hP = contextP.h
	}
	if DefaultOptions == nil {
		call(func() C.int { return C.lr_refresh_create(contextQ.h, hP, C.uint64_t(t), C.int(maxBatch), &r.h) })
	} else {
		call(func() C.int {
			return C.lr_refresh_create_ex(contextQ.h, hP, C.uint64_t(t), C.int(maxBatch), DefaultOptions.ptr(), &r.h)
		})
	}
	runtime.SetFinalizer(r, func(r *Refresh) { C.lr_refresh_destroy(r.h) })
	return r
}

// MaskWords: the 64-bit words of a CKKS mask coefficient at levelStart, ceil(bitlen(Q_levelStart) / 64)
func (r *Refresh) MaskWords(levelStart uint64) int {
	var w C.int
	call(func() C.int { return C.lr_refresh_mask_words(r.h, C.int(levelStart), &w) })
	return int(w)
}

// MaskWordPlanes lays the centred masks out as lr_refresh takes them: word w of coefficient j at planes[w*N + j], two's complement on
// `words` little-endian words.
func MaskWordPlanes(mask []*big.Int, words int) []uint64 {
	n := len(mask)
	planes := make([]uint64, words*n)
	modulus := new(big.Int).Lsh(big.NewInt(1), uint(64*words))
	low := new(big.Int).SetUint64(^uint64(0))
	v, w := new(big.Int), new(big.Int)
	for j, m := range mask {
		v.Set(m)
		if v.Sign() < 0 {
			v.Add(v, modulus)
		}
		for k := 0; k < words; k++ {
			planes[k*n+j] = w.And(v, low).Uint64()
			v.Rsh(v, 64)
		}
	}
	return planes
}

func (r *Refresh) noiseLen(what string, noises ...[]byte) {
	for _, e := range noises {
		if len(e) != int(r.contextQ.N) {
			panic("cannot " + what + ": the compact randomness is N bytes per sampled poly")
		}
	}
}

// CkksGenShares = RefreshProtocol.GenShares of dckks (public_refresh.go:66-92): c1, crs and the shares in the NTT domain, sk in
// NTT + Montgomery form, planes = MaskWordPlanes(mask, MaskWords(levelStart)).
func (r *Refresh) CkksGenShares(sk *Poly, levelStart uint64, c1, crs *Poly, planes []uint64, e0, e1 []byte, shareDecrypt, shareRecrypt *Poly) {
	r.noiseLen("CkksGenShares", e0, e1)
	if len(planes) != r.MaskWords(levelStart)*int(r.contextQ.N) {
		panic("cannot CkksGenShares: the mask is MaskWords(levelStart) word planes of N words")
	}
	r.contextQ.use(sk, c1, crs)
	r.contextQ.want(shareDecrypt, shareRecrypt)
	call(func() C.int {
		return C.lr_refresh_ckks_shares(r.h, C.int(levelStart), sk.d, c1.d, crs.d, (*C.uint64_t)(unsafe.Pointer(&planes[0])), bytePtr(e0), bytePtr(e1), 1, shareDecrypt.d, shareRecrypt.d)
	})
	done(shareDecrypt, shareRecrypt)
}

// CkksRecode = Recode (public_refresh.go:108-139): polIn at levelStart, polOut over all of Q, both in the NTT domain; polOut may be polIn.
func (r *Refresh) CkksRecode(levelStart uint64, polIn, polOut *Poly) {
	r.contextQ.use(polIn)
	r.contextQ.want(polOut)
	call(func() C.int { return C.lr_refresh_ckks_recode(r.h, C.int(levelStart), polIn.d, polOut.d) })
	done(polOut)
}

// CkksFinalize = Decrypt (:103), Recode (:108) and Recrypt's Add (:144) into out0 over all of Q; ct[1] = crs.CopyNew() stays the caller's.
func (r *Refresh) CkksFinalize(levelStart uint64, c0, shareDecrypt, shareRecrypt, out0 *Poly) {
	r.contextQ.use(c0, shareDecrypt, shareRecrypt)
	r.contextQ.want(out0)
	call(func() C.int {
		return C.lr_refresh_ckks_finalize(r.h, C.int(levelStart), c0.d, shareDecrypt.d, shareRecrypt.d, out0.d)
	})
	done(out0)
}

// BfvGenShares = RefreshProtocol.GenShares of dbfv (public_refresh.go:105-160): c1 and the shares in the coefficient domain over Q, crs
// over Q||P, sk over Q||P in NTT + Montgomery form, mask = contextT.NewUniformPoly().Coeffs[0].
func (r *Refresh) BfvGenShares(sk, c1, crs *Poly, mask []uint64, e0, e1 []byte, shareDecrypt, shareRecrypt *Poly) {
	r.noiseLen("BfvGenShares", e0, e1)
	if len(mask) != int(r.contextQ.N) {
		panic("cannot BfvGenShares: the mask is N values below t")
	}
	r.contextQ.use(sk, c1, crs)
	r.contextQ.want(shareDecrypt, shareRecrypt)
	call(func() C.int {
		return C.lr_refresh_bfv_shares(r.h, sk.d, c1.d, crs.d, (*C.uint64_t)(unsafe.Pointer(&mask[0])), bytePtr(e0), bytePtr(e1), 1, shareDecrypt.d, shareRecrypt.d)
	})
	done(shareDecrypt, shareRecrypt)
}

// BfvFinalize = Finalize (public_refresh.go:193-197): out0 = lift(Scale(c0 + shareDecrypt)) + shareRecrypt, out1 = ModDownPQ(crs).
func (r *Refresh) BfvFinalize(c0, crs, shareDecrypt, shareRecrypt, out0, out1 *Poly) {
	r.contextQ.use(c0, crs, shareDecrypt, shareRecrypt)
	r.contextQ.want(out0, out1)
	call(func() C.int {
		return C.lr_refresh_bfv_finalize(r.h, c0.d, crs.d, shareDecrypt.d, shareRecrypt.d, out0.d, out1.d)
	})
	done(out0, out1)
}

// Aggregate = Aggregate of both protocols over all of `shares` in their order, over limbs 0 .. level; out may be one of the shares.
func (r *Refresh) Aggregate(level uint64, shares []*Poly, out *Poly) {
	r.contextQ.use(shares...)
	r.contextQ.want(out)
	n := len(shares)
	raw := C.malloc(C.size_t(n) * C.size_t(unsafe.Sizeof(uintptr(0))))
	defer C.free(raw)
	arr := polyArray(raw, n)
	for i := range shares {
		arr[i] = shares[i].d
	}
	call(func() C.int { return C.lr_refresh_aggregate(r.h, C.int(level), (**C.lr_poly)(raw), C.int(n), out.d) })
	done(out)
}

// The Device forms: the same randomness in device memory for `batch` ciphertexts, stream-ordered on contextQ's stream, no host copy and
// no synchronisation; the polys must be resident (Poly.Pin) and hold `batch` polys.
func (r *Refresh) CkksGenSharesDevice(sk *Poly, levelStart uint64, c1, crs *Poly, planes, e0, e1 unsafe.Pointer, batch int, shareDecrypt, shareRecrypt *Poly) {
	r.contextQ.use(sk, c1, crs)
	r.contextQ.want(shareDecrypt, shareRecrypt)
	call(func() C.int {
		return C.lr_refresh_ckks_shares_device(r.h, C.int(levelStart), sk.d, c1.d, crs.d, planes, e0, e1, C.int(batch), shareDecrypt.d, shareRecrypt.d)
	})
}

func (r *Refresh) BfvGenSharesDevice(sk, c1, crs *Poly, mask, e0, e1 unsafe.Pointer, batch int, shareDecrypt, shareRecrypt *Poly) {
	r.contextQ.use(sk, c1, crs)
	r.contextQ.want(shareDecrypt, shareRecrypt)
	call(func() C.int {
		return C.lr_refresh_bfv_shares_device(r.h, sk.d, c1.d, crs.d, mask, e0, e1, C.int(batch), shareDecrypt.d, shareRecrypt.d)
	})
}
