package ring

// #include <stdlib.h>
// #include "lattigo_ring.h"
import "C"

import (
	"runtime"
	"unsafe"
)

// CkksEncryptor: what ckks's newEncryptor builds (ckks/encryptor.go:100-119) -- the basis extender, three pool polys over Q||P, the
// matrixTernaryMontgomery rows -- with pkEncryptor.encrypt (:179-237) and skEncryptor.encrypt (:318-362) on the device, after the
// sampling.  The randomness is the samplers' decisions in the compact form of BfvEncryptor, recorded by the same samplers
// (SampleTernaryBits, KYSampler.SampleCompact in bfv_encryptor.go): N/4 + 2N bytes per public-key ciphertext cross to the device
// instead of three polys over Q||P.  Plaintext and ciphertext are in the NTT domain over limbs 0 .. level; limbs above level are not
// touched.  A Go Poly is one polynomial, so the slice forms encrypt one ciphertext per call; the Device forms take the randomness in
// device memory.  contextP nil is upstream's "modulus P is empty": only the fast forms work.
type CkksEncryptor struct {
	contextQ, contextP *Context
	MaxBatch           int
	h                  *C.lr_ckks_encryptor
}

func NewCkksEncryptor(contextQ, contextP *Context, maxBatch int) *CkksEncryptor {
	e := &CkksEncryptor{contextQ: contextQ, contextP: contextP, MaxBatch: maxBatch}
	var hP *C.lr_context
	if contextP != nil {
		hP = contextP.h
	}
	if DefaultOptions == nil {
		call(func() C.int { return C.lr_ckks_encryptor_create(contextQ.h, hP, C.int(maxBatch), &e.h) })
	} else {
		call(func() C.int {
			return C.lr_ckks_encryptor_create_ex(contextQ.h, hP, C.int(maxBatch), DefaultOptions.ptr(), &e.h)
		})
	}
	runtime.SetFinalizer(e, func(e *CkksEncryptor) { C.lr_ckks_encryptor_destroy(e.h) })
	return e
}

// EncryptPk = pkEncryptor.encrypt: pk over Q||P in NTT + Montgomery form (fast: its first |Q| limbs are read), uCoeffs / uSigns the
// two bit planes of N/8 bytes, e0 / e1 N bytes each, plaintext and ctOut in the NTT domain with at least level+1 limbs.
func (e *CkksEncryptor) EncryptPk(level uint64, pk [2]*Poly, uCoeffs, uSigns, e0, e1 []byte, plaintext *Poly, ctOut [2]*Poly, fast bool) {
	q := e.contextQ
	n := int(q.N)
	if len(uCoeffs) != n>>3 || len(uSigns) != n>>3 || len(e0) != n || len(e1) != n {
		panic("cannot EncryptPk: the compact randomness is N/8 bytes per bit plane and N bytes per sampled poly")
	}
	q.use(pk[0], pk[1], plaintext)
	q.want(ctOut[0], ctOut[1])
	call(func() C.int {
		return C.lr_ckks_encryptor_encrypt_pk(e.h, cBool(fast), C.int(level), pk[0].d, pk[1].d, bytePtr(uCoeffs), bytePtr(uSigns), bytePtr(e0), bytePtr(e1), plaintext.d, 1, ctOut[0].d, ctOut[1].d)
	})
	done(ctOut[0], ctOut[1])
}

// EncryptSk = skEncryptor.encrypt with crp the uniform poly in the NTT domain (over Q||P, fast: over Q); crp is not modified.
func (e *CkksEncryptor) EncryptSk(level uint64, sk, crp *Poly, noise []byte, plaintext *Poly, ctOut [2]*Poly, fast bool) {
	q := e.contextQ
	if len(noise) != int(q.N) {
		panic("cannot EncryptSk: the compact randomness is N bytes per sampled poly")
	}
	q.use(sk, crp, plaintext)
	q.want(ctOut[0], ctOut[1])
	call(func() C.int {
		return C.lr_ckks_encryptor_encrypt_sk(e.h, cBool(fast), C.int(level), sk.d, crp.d, bytePtr(noise), plaintext.d, 1, ctOut[0].d, ctOut[1].d)
	})
	done(ctOut[0], ctOut[1])
}

// EncryptPkDevice / EncryptSkDevice: the same bytes in device memory, stream-ordered on contextQ's stream, no host copy and no
// synchronisation; the polys must be resident (Poly.Pin).
func (e *CkksEncryptor) EncryptPkDevice(level uint64, pk [2]*Poly, uCoeffs, uSigns, e0, e1 unsafe.Pointer, plaintext *Poly, ctOut [2]*Poly, fast bool) {
	q := e.contextQ
	q.use(pk[0], pk[1], plaintext)
	q.want(ctOut[0], ctOut[1])
	call(func() C.int {
		return C.lr_ckks_encryptor_encrypt_pk_device(e.h, cBool(fast), C.int(level), pk[0].d, pk[1].d, uCoeffs, uSigns, e0, e1, plaintext.d, 1, ctOut[0].d, ctOut[1].d)
	})
}

func (e *CkksEncryptor) EncryptSkDevice(level uint64, sk, crp *Poly, noise unsafe.Pointer, plaintext *Poly, ctOut [2]*Poly, fast bool) {
	q := e.contextQ
	q.use(sk, crp, plaintext)
	q.want(ctOut[0], ctOut[1])
	call(func() C.int {
		return C.lr_ckks_encryptor_encrypt_sk_device(e.h, cBool(fast), C.int(level), sk.d, crp.d, noise, plaintext.d, 1, ctOut[0].d, ctOut[1].d)
	})
}
