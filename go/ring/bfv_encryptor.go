package ring

// #include <stdlib.h>
// #include "lattigo_ring.h"
import "C"

import (
	"crypto/rand"
	"runtime"
	"unsafe"
)

// BfvEncryptor: what bfv's newEncryptor builds (bfv/encryptor.go:100-119) -- the basis extender, three pool polys over Q||P, the
// matrixTernaryMontgomery rows -- with pkEncryptor.encrypt (:169-223) and skEncryptor.encrypt (:306-345) on the device, after the
// sampling.  The randomness is the samplers' decisions in compact form (SampleTernaryBits, KYSampler.SampleCompact,
// Context.SampleGaussianCompact below): N/4 + 2N bytes per public-key ciphertext cross to the device instead of three polys.
// A Go Poly is one polynomial, so the slice forms encrypt one ciphertext per call; the Device forms take maxBatch ciphertexts'
// randomness in device memory.  contextP nil is upstream's "modulus P is empty": only the fast forms work.
type BfvEncryptor struct {
	contextQ, contextP *Context
	MaxBatch           int
	h                  *C.lr_bfv_encryptor
}

func NewBfvEncryptor(contextQ, contextP *Context, maxBatch int) *BfvEncryptor {
	e := &BfvEncryptor{contextQ: contextQ, contextP: contextP, MaxBatch: maxBatch}
	var hP *C.lr_context
	if contextP != nil {
		hP = contextP.h
	}
	if DefaultOptions == nil {
		call(func() C.int { return C.lr_bfv_encryptor_create(contextQ.h, hP, C.int(maxBatch), &e.h) })
	} else {
		call(func() C.int {
			return C.lr_bfv_encryptor_create_ex(contextQ.h, hP, C.int(maxBatch), DefaultOptions.ptr(), &e.h)
		})
	}
	runtime.SetFinalizer(e, func(e *BfvEncryptor) { C.lr_bfv_encryptor_destroy(e.h) })
	return e
}

func bytePtr(b []byte) *C.uint8_t {
	return (*C.uint8_t)(unsafe.Pointer(&b[0]))
}

// EncryptPk = pkEncryptor.encrypt: pk over Q||P in NTT + Montgomery form (fast: its first |Q| limbs are read), uCoeffs / uSigns the
// two bit planes of N/8 bytes, e0 / e1 N bytes each, plaintext and ctOut over Q in the coefficient domain.
func (e *BfvEncryptor) EncryptPk(pk [2]*Poly, uCoeffs, uSigns, e0, e1 []byte, plaintext *Poly, ctOut [2]*Poly, fast bool) {
	q := e.contextQ
	n := int(q.N)
	if len(uCoeffs) != n>>3 || len(uSigns) != n>>3 || len(e0) != n || len(e1) != n {
		panic("cannot EncryptPk: the compact randomness is N/8 bytes per bit plane and N bytes per sampled poly")
	}
	q.use(pk[0], pk[1], plaintext)
	q.want(ctOut[0], ctOut[1])
	call(func() C.int {
		return C.lr_bfv_encrypt_pk(e.h, cBool(fast), pk[0].d, pk[1].d, bytePtr(uCoeffs), bytePtr(uSigns), bytePtr(e0), bytePtr(e1), plaintext.d, 1, ctOut[0].d, ctOut[1].d)
	})
	done(ctOut[0], ctOut[1])
}

// EncryptSk = skEncryptor.encrypt with crp the uniform poly in the NTT domain (over Q||P, fast: over Q); crp is not modified.
func (e *BfvEncryptor) EncryptSk(sk, crp *Poly, noise []byte, plaintext *Poly, ctOut [2]*Poly, fast bool) {
	q := e.contextQ
	if len(noise) != int(q.N) {
		panic("cannot EncryptSk: the compact randomness is N bytes per sampled poly")
	}
	q.use(sk, crp, plaintext)
	q.want(ctOut[0], ctOut[1])
	call(func() C.int {
		return C.lr_bfv_encrypt_sk(e.h, cBool(fast), sk.d, crp.d, bytePtr(noise), plaintext.d, 1, ctOut[0].d, ctOut[1].d)
	})
	done(ctOut[0], ctOut[1])
}

// EncryptPkDevice / EncryptSkDevice: the same bytes in device memory, stream-ordered on contextQ's stream, no host copy and no
// synchronisation; the polys must be resident (Poly.Pin).
func (e *BfvEncryptor) EncryptPkDevice(pk [2]*Poly, uCoeffs, uSigns, e0, e1 unsafe.Pointer, plaintext *Poly, ctOut [2]*Poly, fast bool) {
	q := e.contextQ
	q.use(pk[0], pk[1], plaintext)
	q.want(ctOut[0], ctOut[1])
	call(func() C.int {
		return C.lr_bfv_encrypt_pk_device(e.h, cBool(fast), pk[0].d, pk[1].d, uCoeffs, uSigns, e0, e1, plaintext.d, 1, ctOut[0].d, ctOut[1].d)
	})
}

func (e *BfvEncryptor) EncryptSkDevice(sk, crp *Poly, noise unsafe.Pointer, plaintext *Poly, ctOut [2]*Poly, fast bool) {
	q := e.contextQ
	q.use(sk, crp, plaintext)
	q.want(ctOut[0], ctOut[1])
	call(func() C.int {
		return C.lr_bfv_encrypt_sk_device(e.h, cBool(fast), sk.d, crp.d, noise, plaintext.d, 1, ctOut[0].d, ctOut[1].d)
	})
}

// BfvDecryptor: bfv.NewDecryptor's pool (bfv/decryptor.go:28-45) with decryptor.Decrypt (:55-75) on the device.
type BfvDecryptor struct {
	contextQ *Context
	MaxBatch int
	h        *C.lr_bfv_decryptor
}

func NewBfvDecryptor(contextQ *Context, maxBatch int) *BfvDecryptor {
	d := &BfvDecryptor{contextQ: contextQ, MaxBatch: maxBatch}
	call(func() C.int { return C.lr_bfv_decryptor_create(contextQ.h, C.int(maxBatch), &d.h) })
	runtime.SetFinalizer(d, func(d *BfvDecryptor) { C.lr_bfv_decryptor_destroy(d.h) })
	return d
}

// Decrypt: ct = the components of the ciphertext (degree len(ct) - 1), sk in NTT + Montgomery form (its first |Q| limbs are read);
// ptOut may be the top component.
func (d *BfvDecryptor) Decrypt(ct []*Poly, sk, ptOut *Poly) {
	q := d.contextQ
	q.use(ct...)
	q.use(sk)
	q.want(ptOut)
	n := len(ct)
	raw := C.malloc(C.size_t(n) * C.size_t(unsafe.Sizeof(uintptr(0))))
	defer C.free(raw)
	arr := polyArray(raw, n)
	for i := range ct {
		arr[i] = ct[i].d
	}
	call(func() C.int { return C.lr_bfv_decrypt(d.h, (**C.lr_poly)(raw), C.int(n-1), sk.d, ptOut.d, 1) })
	done(ptOut)
}

// ---- compact samplers: the decisions of the upstream samplers (gaussianSampler.go, ternarySampler.go, kept from upstream) before
// they are written into limbs.  crypto/rand is consumed exactly as upstream consumes it.

// SampleCompact runs upstream's kysampling for the N coefficients of one poly, as KYSampler.Sample does (gaussianSampler.go:230-251),
// and writes coeff | sign<<7 per coefficient instead of the residues.
func (kys *KYSampler) SampleCompact(dst []byte) {
	if uint64(len(dst)) != kys.context.N {
		panic("cannot SampleCompact: one byte per coefficient")
	}
	var coeff, sign uint64
	randomBytes := make([]byte, 8)
	pointer := uint8(0)
	if _, err := rand.Read(randomBytes); err != nil {
		panic("crypto rand error")
	}
	for i := range dst {
		coeff, sign, randomBytes, pointer = kysampling(kys.Matrix, randomBytes, pointer)
		dst[i] = byte(coeff) | byte(sign)<<7
	}
}

// SampleGaussianCompact is the ziggurat of Context.SampleGaussianAndAdd (gaussianSampler.go:38-64) with the same rejection at
// bound, writing coeff | sign<<7; bound must stay below 128 (upstream's is 6 sigma = 19).
func (context *Context) SampleGaussianCompact(dst []byte, sigma float64, bound uint64) {
	if uint64(len(dst)) != context.N || bound > 127 {
		panic("cannot SampleGaussianCompact: one byte per coefficient, seven bits of magnitude")
	}
	var coeffFlo float64
	var coeffInt, sign uint64
	randomBytes := make([]byte, 1024)
	if _, err := rand.Read(randomBytes); err != nil {
		panic("crypto rand error")
	}
	for i := range dst {
		for {
			coeffFlo, sign, randomBytes = normFloat64(randomBytes)
			if coeffInt = uint64(coeffFlo * sigma); coeffInt <= bound {
				break
			}
		}
		dst[i] = byte(coeffInt) | byte(sign)<<7
	}
}

// SampleTernaryBits is sampleTernary's randomness at p = 0.5 (ternarySampler.go:157-166): the coefficient plane, then the sign plane,
// N/8 bytes each.
func SampleTernaryBits(coeffs, signs []byte) {
	if _, err := rand.Read(coeffs); err != nil {
		panic("crypto rand error")
	}
	if _, err := rand.Read(signs); err != nil {
		panic("crypto rand error")
	}
}
