package ring

// #include <stdlib.h>
// #include "lattigo_ring.h"
import "C"

import (
	"runtime"
	"unsafe"
)

// Collective: what NewCKSProtocol and NewPCKSProtocol of dckks and dbfv build (dckks/keyswitching.go:28-49,
// dckks/public_keyswitching.go:28-49, dbfv/keyswitching.go:38-59, dbfv/public_keyswitching.go:76-97) -- the basis extender, tmp,
// share0tmp and share1tmp over Q||P, MForm(P) -- with the four GenShare bodies, AggregateShares and KeySwitch on the device, after the
// sampling.  The randomness is the samplers' decisions in the compact form of BfvEncryptor, recorded by the same samplers
// (SampleTernaryBits, KYSampler.SampleCompact in bfv_encryptor.go): N bytes per CKS share and N/4 + 2N per PCKS share cross to the
// device instead of polys over Q||P, and the ciphertext stays where the evaluator left it.  The smudging sampler and the regular one
// differ only in which KYSampler records the bytes; a magnitude is at most 127 (sigma_smudge <= 21 with upstream's bound int(6 sigma)).
// A Go Poly is one polynomial, so the slice forms make one share per call; the Device forms take maxBatch ciphertexts' randomness in
// device memory.
type Collective struct {
	contextQ, contextP *Context
	MaxBatch           int
	h                  *C.lr_collective
}

func NewCollective(contextQ, contextP *Context, maxBatch int) *Collective {
	if contextP == nil {
		panic("cannot NewCollective: modulus P is empty")
	}
	c := &Collective{contextQ: contextQ, contextP: contextP, MaxBatch: maxBatch}
	if DefaultOptions == nil {
		call(func() C.int { return C.lr_collective_create(contextQ.h, contextP.h, C.int(maxBatch), &c.h) })
	} else {
		call(func() C.int {
			return C.lr_collective_create_ex(contextQ.h, contextP.h, C.int(maxBatch), DefaultOptions.ptr(), &c.h)
		})
	}
	runtime.SetFinalizer(c, func(c *Collective) { C.lr_collective_destroy(c.h) })
	return c
}

func (c *Collective) noiseLen(what string, noises ...[]byte) {
	for _, e := range noises {
		if len(e) != int(c.contextQ.N) {
			panic("cannot " + what + ": the compact randomness is N bytes per sampled poly")
		}
	}
}

// CkksCksShare = CKSProtocol.GenShare of dckks (keyswitching.go:62-94) at `level`: c1 and shareOut in the NTT domain, the keys in
// NTT + Montgomery form (their first |Q| limbs are read), noise N bytes of the smudging sampler.
func (c *Collective) CkksCksShare(level uint64, skInput, skOutput, c1 *Poly, noise []byte, shareOut *Poly) {
	c.noiseLen("CkksCksShare", noise)
	c.contextQ.use(skInput, skOutput, c1)
	c.contextQ.want(shareOut)
	call(func() C.int {
		return C.lr_collective_ckks_cks_share(c.h, C.int(level), skInput.d, skOutput.d, c1.d, bytePtr(noise), 1, shareOut.d)
	})
	done(shareOut)
}

// BfvCksShare = CKSProtocol.GenShare of dbfv (keyswitching.go:74-109): c1 and shareOut in the coefficient domain over Q.
func (c *Collective) BfvCksShare(skInput, skOutput, c1 *Poly, noise []byte, shareOut *Poly) {
	c.noiseLen("BfvCksShare", noise)
	c.contextQ.use(skInput, skOutput, c1)
	c.contextQ.want(shareOut)
	call(func() C.int {
		return C.lr_collective_bfv_cks_share(c.h, skInput.d, skOutput.d, c1.d, bytePtr(noise), 1, shareOut.d)
	})
	done(shareOut)
}

func (c *Collective) planes(what string, uCoeffs, uSigns []byte) {
	n := int(c.contextQ.N)
	if len(uCoeffs) != n>>3 || len(uSigns) != n>>3 {
		panic("cannot " + what + ": the compact randomness is N/8 bytes per bit plane")
	}
}

// CkksPcksShare = PCKSProtocol.GenShare of dckks (public_keyswitching.go:63-93): pk over Q||P, uCoeffs / uSigns the two bit planes of u,
// e0 the smudging sampler's bytes and e1 the regular sampler's.
func (c *Collective) CkksPcksShare(level uint64, sk *Poly, pk [2]*Poly, c1 *Poly, uCoeffs, uSigns, e0, e1 []byte, shareOut [2]*Poly) {
	c.planes("CkksPcksShare", uCoeffs, uSigns)
	c.noiseLen("CkksPcksShare", e0, e1)
	c.contextQ.use(sk, pk[0], pk[1], c1)
	c.contextQ.want(shareOut[0], shareOut[1])
	call(func() C.int {
		return C.lr_collective_ckks_pcks_share(c.h, C.int(level), sk.d, pk[0].d, pk[1].d, c1.d, bytePtr(uCoeffs), bytePtr(uSigns), bytePtr(e0), bytePtr(e1), 1, shareOut[0].d, shareOut[1].d)
	})
	done(shareOut[0], shareOut[1])
}

// BfvPcksShare = PCKSProtocol.GenShare of dbfv (public_keyswitching.go:111-148).
func (c *Collective) BfvPcksShare(sk *Poly, pk [2]*Poly, c1 *Poly, uCoeffs, uSigns, e0, e1 []byte, shareOut [2]*Poly) {
	c.planes("BfvPcksShare", uCoeffs, uSigns)
	c.noiseLen("BfvPcksShare", e0, e1)
	c.contextQ.use(sk, pk[0], pk[1], c1)
	c.contextQ.want(shareOut[0], shareOut[1])
	call(func() C.int {
		return C.lr_collective_bfv_pcks_share(c.h, sk.d, pk[0].d, pk[1].d, c1.d, bytePtr(uCoeffs), bytePtr(uSigns), bytePtr(e0), bytePtr(e1), 1, shareOut[0].d, shareOut[1].d)
	})
	done(shareOut[0], shareOut[1])
}

// Aggregate = AggregateShares over all of `shares` in their order and, with base = ct[0], KeySwitch's Add, in one pass over limbs
// 0 .. level; one share and a nil base is KeySwitch's Copy.  out may be base or one of the shares.
func (c *Collective) Aggregate(level uint64, base *Poly, shares []*Poly, out *Poly) {
	c.contextQ.use(shares...)
	var hb *C.lr_poly
	if base != nil {
		c.contextQ.use(base)
		hb = base.d
	}
	c.contextQ.want(out)
	n := len(shares)
	raw := C.malloc(C.size_t(n) * C.size_t(unsafe.Sizeof(uintptr(0))))
	defer C.free(raw)
	arr := polyArray(raw, n)
	for i := range shares {
		arr[i] = shares[i].d
	}
	call(func() C.int { return C.lr_collective_aggregate(c.h, C.int(level), hb, (**C.lr_poly)(raw), C.int(n), out.d) })
	done(out)
}

// The Device forms: the same bytes in device memory for `batch` ciphertexts, stream-ordered on contextQ's stream, no host copy and no
// synchronisation; the polys must be resident (Poly.Pin) and hold `batch` polys.
func (c *Collective) CkksCksShareDevice(level uint64, skInput, skOutput, c1 *Poly, noise unsafe.Pointer, batch int, shareOut *Poly) {
	c.contextQ.use(skInput, skOutput, c1)
	c.contextQ.want(shareOut)
	call(func() C.int {
		return C.lr_collective_ckks_cks_share_device(c.h, C.int(level), skInput.d, skOutput.d, c1.d, noise, C.int(batch), shareOut.d)
	})
}

func (c *Collective) BfvCksShareDevice(skInput, skOutput, c1 *Poly, noise unsafe.Pointer, batch int, shareOut *Poly) {
	c.contextQ.use(skInput, skOutput, c1)
	c.contextQ.want(shareOut)
	call(func() C.int {
		return C.lr_collective_bfv_cks_share_device(c.h, skInput.d, skOutput.d, c1.d, noise, C.int(batch), shareOut.d)
	})
}

func (c *Collective) CkksPcksShareDevice(level uint64, sk *Poly, pk [2]*Poly, c1 *Poly, uCoeffs, uSigns, e0, e1 unsafe.Pointer, batch int, shareOut [2]*Poly) {
	c.contextQ.use(sk, pk[0], pk[1], c1)
	c.contextQ.want(shareOut[0], shareOut[1])
	call(func() C.int {
		return C.lr_collective_ckks_pcks_share_device(c.h, C.int(level), sk.d, pk[0].d, pk[1].d, c1.d, uCoeffs, uSigns, e0, e1, C.int(batch), shareOut[0].d, shareOut[1].d)
	})
}

func (c *Collective) BfvPcksShareDevice(sk *Poly, pk [2]*Poly, c1 *Poly, uCoeffs, uSigns, e0, e1 unsafe.Pointer, batch int, shareOut [2]*Poly) {
	c.contextQ.use(sk, pk[0], pk[1], c1)
	c.contextQ.want(shareOut[0], shareOut[1])
	call(func() C.int {
		return C.lr_collective_bfv_pcks_share_device(c.h, sk.d, pk[0].d, pk[1].d, c1.d, uCoeffs, uSigns, e0, e1, C.int(batch), shareOut[0].d, shareOut[1].d)
	})
}
