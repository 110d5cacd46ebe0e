package ring

// #include <stdlib.h>
// #include "lattigo_ring.h"
import "C"

import (
	"runtime"
	"unsafe"
)

// KeyGenerator: what NewKeyGenerator builds (ckks/keygen.go:79-94, bfv/keygen.go:70-84) -- the pool over Q||P -- with GenSecretKey,
// GenPublicKey and newSwitchingKey (ckks/keygen.go:282-338, bfv/keygen.go:285-333) on the device, after the sampling.  The randomness
// is the samplers' decisions in the compact form of BfvEncryptor, recorded by the same samplers (SampleTernaryBits,
// KYSampler.SampleCompact in bfv_encryptor.go): beta N bytes per switching key cross to the device instead of beta polys over Q||P, and
// evakey[i][0] is made where the key switch reads it.  Secret and public keys are polys over Q||P bound to contextQ; a switching key is
// the image CkksPlan.SwitchingKeyImage lays out (batch 2 beta), whose odd members hold the caller's uniform polys on entry and are not
// written.  contextP nil is upstream's "modulus P is empty": only the secret key and the public key.
type KeyGenerator struct {
	contextQ, contextP *Context
	MaxBatch           int
	h                  *C.lr_keygen
}

func NewKeyGenerator(contextQ, contextP *Context, maxBatch int) *KeyGenerator {
	g := &KeyGenerator{contextQ: contextQ, contextP: contextP, MaxBatch: maxBatch}
	var hP *C.lr_context
	if contextP != nil {
		hP = contextP.h
	}
	if DefaultOptions == nil {
		call(func() C.int { return C.lr_keygen_create(contextQ.h, hP, C.int(maxBatch), &g.h) })
	} else {
		call(func() C.int { return C.lr_keygen_create_ex(contextQ.h, hP, C.int(maxBatch), DefaultOptions.ptr(), &g.h) })
	}
	runtime.SetFinalizer(g, func(g *KeyGenerator) { C.lr_keygen_destroy(g.h) })
	return g
}

// Beta = params.Beta(): ceil(|Q| / |P|), the digits of a switching key.
func (g *KeyGenerator) Beta() int {
	if g.contextP == nil {
		panic("cannot Beta: modulus P is empty")
	}
	nQ, nP := len(g.contextQ.Modulus), len(g.contextP.Modulus)
	return (nQ + nP - 1) / nP
}

// NewSwitchingKeyImage allocates the device image of one SwitchingKey and uploads the caller's uniform polys (evakey[i][1], what
// upstream's NewUniformPoly drew) into its odd members; the even members are the outputs of the three calls below.
func (g *KeyGenerator) NewSwitchingKeyImage(uniform []*Poly) *Poly {
	limbs := len(uniform[0].Coeffs)
	img := &Poly{resident: true, dLimbs: limbs}
	call(func() C.int { return C.lr_poly_alloc(g.contextQ.h, C.int(limbs), C.int(2*len(uniform)), &img.d) })
	for i, a := range uniform {
		a.hostView()
		a.uploadTo(img.d, 2*i+1)
	}
	runtime.SetFinalizer(img, func(q *Poly) { C.lr_poly_free(q.d) })
	return img
}

// DownloadKey copies the even members of an image into evakey[i][0] on the host (marshalling, SetRelinKeys / SetRotKey of another party).
func (g *KeyGenerator) DownloadKey(image *Poly, evakey [][2]*Poly) {
	for i := range evakey {
		dst := evakey[i][0]
		for j := range dst.Coeffs {
			member, limb := C.int(2*i), C.int(j)
			p := (*C.uint64_t)(unsafe.Pointer(&dst.Coeffs[j][0]))
			call(func() C.int { return C.lr_poly_download_limb(image.d, member, limb, p) })
		}
	}
}

func keyHandles(images []*Poly) **C.lr_poly {
	hs := make([]*C.lr_poly, len(images)) // C pointers in Go memory: allowed to cross for the duration of the call
	for i, img := range images {
		hs[i] = img.d
	}
	return (**C.lr_poly)(unsafe.Pointer(&hs[0]))
}

func (g *KeyGenerator) noiseLen(keys int, noise []byte, what string) {
	if len(noise) != keys*g.Beta()*int(g.contextQ.N) {
		panic("cannot " + what + ": the compact randomness is beta x N bytes per switching key")
	}
}

// GenSecretKey = SampleTernaryMontgomeryNTTNew (ckks/keygen.go:104) from the two bit planes of N/8 bytes.
func (g *KeyGenerator) GenSecretKey(coeffs, signs []byte, sk *Poly) {
	q := g.contextQ
	if len(coeffs) != int(q.N)>>3 || len(signs) != int(q.N)>>3 {
		panic("cannot GenSecretKey: the compact randomness is N/8 bytes per bit plane")
	}
	q.want(sk)
	call(func() C.int { return C.lr_keygen_secret_key(g.h, bytePtr(coeffs), bytePtr(signs), 1, sk.d) })
	done(sk)
}

// GenPublicKey (ckks/keygen.go:138-151): pk[1] = the caller's uniform poly, pk[0] the output; noise N bytes.
func (g *KeyGenerator) GenPublicKey(sk *Poly, noise []byte, pk [2]*Poly) {
	q := g.contextQ
	if len(noise) != int(q.N) {
		panic("cannot GenPublicKey: the compact randomness is N bytes per sampled poly")
	}
	q.use(sk, pk[1])
	q.want(pk[0])
	call(func() C.int { return C.lr_keygen_public_key(g.h, sk.d, bytePtr(noise), 1, pk[0].d, pk[1].d) })
	done(pk[0])
}

// GenSwitchingKeys = newSwitchingKey for len(images) keys from skIn to skOut (GenSwitchingKey, ckks/keygen.go:247-258).
func (g *KeyGenerator) GenSwitchingKeys(skIn, skOut *Poly, noise []byte, images []*Poly) {
	g.noiseLen(len(images), noise, "GenSwitchingKeys")
	g.contextQ.use(skIn, skOut)
	call(func() C.int {
		return C.lr_keygen_switching_keys(g.h, skIn.d, skOut.d, bytePtr(noise), C.int(len(images)), keyHandles(images))
	})
}

// GenRelinKeys: image i switches from sk^(i+2); one image is ckks GenRelinKey (:192-205), maxDegree images bfv GenRelinKey (:172-196).
func (g *KeyGenerator) GenRelinKeys(sk *Poly, noise []byte, images []*Poly) {
	g.noiseLen(len(images), noise, "GenRelinKeys")
	g.contextQ.use(sk)
	call(func() C.int { return C.lr_keygen_relin_keys(g.h, sk.d, C.int(len(images)), bytePtr(noise), keyHandles(images)) })
}

// GenRotationKeys = genrotKey (ckks/keygen.go:487-494) for each Galois element, one call for all of them.
func (g *KeyGenerator) GenRotationKeys(sk *Poly, galEls []uint64, noise []byte, images []*Poly) {
	if len(galEls) != len(images) {
		panic("cannot GenRotationKeys: one image per Galois element")
	}
	g.noiseLen(len(images), noise, "GenRotationKeys")
	g.contextQ.use(sk)
	call(func() C.int {
		return C.lr_keygen_rotation_keys(g.h, sk.d, (*C.uint64_t)(unsafe.Pointer(&galEls[0])), C.int(len(images)), bytePtr(noise), keyHandles(images))
	})
}

// The Device forms: the same bytes in device memory, stream-ordered on contextQ's stream, no host copy and no synchronisation; the
// polys must be resident (Poly.Pin).
func (g *KeyGenerator) GenSecretKeyDevice(coeffs, signs unsafe.Pointer, sk *Poly) {
	g.contextQ.want(sk)
	call(func() C.int { return C.lr_keygen_secret_key_device(g.h, coeffs, signs, 1, sk.d) })
}

func (g *KeyGenerator) GenPublicKeyDevice(sk *Poly, noise unsafe.Pointer, pk [2]*Poly) {
	g.contextQ.use(sk, pk[1])
	g.contextQ.want(pk[0])
	call(func() C.int { return C.lr_keygen_public_key_device(g.h, sk.d, noise, 1, pk[0].d, pk[1].d) })
}

func (g *KeyGenerator) GenSwitchingKeysDevice(skIn, skOut *Poly, noise unsafe.Pointer, images []*Poly) {
	g.contextQ.use(skIn, skOut)
	call(func() C.int {
		return C.lr_keygen_switching_keys_device(g.h, skIn.d, skOut.d, noise, C.int(len(images)), keyHandles(images))
	})
}

func (g *KeyGenerator) GenRelinKeysDevice(sk *Poly, noise unsafe.Pointer, images []*Poly) {
	g.contextQ.use(sk)
	call(func() C.int { return C.lr_keygen_relin_keys_device(g.h, sk.d, C.int(len(images)), noise, keyHandles(images)) })
}

func (g *KeyGenerator) GenRotationKeysDevice(sk *Poly, galEls []uint64, noise unsafe.Pointer, images []*Poly) {
	g.contextQ.use(sk)
	call(func() C.int {
		return C.lr_keygen_rotation_keys_device(g.h, sk.d, (*C.uint64_t)(unsafe.Pointer(&galEls[0])), C.int(len(images)), noise, keyHandles(images))
	})
}
