// Replacement bodies for github.com/ldsec/lattigo/ckks (v1.3.1), encryptor.go: this file is added to the package, the module's ring package
// is replaced by go/ring of this repository (INTEGRATION.md section 3), and the upstream bodies of the methods defined here are DELETED
// from encryptor.go (same receivers and signatures: Go has no virtual dispatch, see go/ckks/evaluator_device.go).
//
// NOT COMPILED IN THIS REPOSITORY'S PIPELINE (no Go toolchain in the image); statically checked by tests/test_go_ckks_encryptor.py.
//
// The patch to upstream ckks/encryptor.go, line numbers of v1.3.1:
//
//	delete  pkEncryptor.encrypt  :179-237  -> below: the samplers' decisions in compact form (ring.SampleTernaryBits, KYSampler.SampleCompact
//	                                          twice, in upstream's order u, e0, e1), then ONE call, CkksEncryptor.EncryptPk, at
//	                                          plaintext.Level(); isNTT is set as upstream sets it
//	delete  skEncryptor.encrypt  :318-362  -> below: the noise in compact form (KYSampler.SampleCompact: both branches use the Knuth-Yao
//	                                          sampler), then ONE call, CkksEncryptor.EncryptSk; crp is read only -- upstream's ModDownNTTPQ
//	                                          transforms the P rows of polypool[1] in place, the device works on its own copy of them
//	keep    newEncryptor :100-119 and the eight interface methods of both encryptors -- EncryptNew, Encrypt, EncryptFastNew, EncryptFast
//	        :126-156, :239-267, and EncryptFromCRPNew, EncryptFromCRP, EncryptFromCRPFastNew, EncryptFromCRPFast :158-172 (the public-key
//	        encryptor panics there), :269-298 -- with encryptSample / encryptFromCRP :300-316, which sample or copy the uniform poly into
//	        polypool[1] on the host: every one of them ends in one of the two bodies below
package ckks

import (
	"sync"

	"github.com/ldsec/lattigo/ring"
)

var deviceCkksEncryptors sync.Map // *encryptor -> *ring.CkksEncryptor

func (encryptor *encryptor) dev() *ring.CkksEncryptor {
	if e, ok := deviceCkksEncryptors.Load(encryptor); ok {
		return e.(*ring.CkksEncryptor)
	}
	var contextP *ring.Context
	if encryptor.baseconverter != nil {
		contextP = encryptor.ckksContext.contextP
	}
	e := ring.NewCkksEncryptor(encryptor.ckksContext.contextQ, contextP, 1)
	actual, _ := deviceCkksEncryptors.LoadOrStore(encryptor, e)
	return actual.(*ring.CkksEncryptor)
}

// ReleaseDevice drops the encryptor's device state and its entry in deviceCkksEncryptors.
func (encryptor *encryptor) ReleaseDevice() {
	deviceCkksEncryptors.Delete(encryptor)
}

// encrypt (:179).
func (encryptor *pkEncryptor) encrypt(plaintext *Plaintext, ciphertext *Ciphertext, fast bool) {
	n := len(plaintext.value.Coeffs[0])
	uCoeffs, uSigns := make([]byte, n>>3), make([]byte, n>>3)
	e0, e1 := make([]byte, n), make([]byte, n)
	ring.SampleTernaryBits(uCoeffs, uSigns)
	encryptor.ckksContext.gaussianSampler.SampleCompact(e0)
	encryptor.ckksContext.gaussianSampler.SampleCompact(e1)
	encryptor.dev().EncryptPk(plaintext.Level(), encryptor.pk.pk, uCoeffs, uSigns, e0, e1, plaintext.value, [2]*ring.Poly{ciphertext.value[0], ciphertext.value[1]}, fast)
	ciphertext.isNTT = true
}

// encrypt (:318).
func (encryptor *skEncryptor) encrypt(plaintext *Plaintext, ciphertext *Ciphertext, crp *ring.Poly, fast bool) {
	noise := make([]byte, len(plaintext.value.Coeffs[0]))
	encryptor.ckksContext.gaussianSampler.SampleCompact(noise)
	encryptor.dev().EncryptSk(plaintext.Level(), encryptor.sk.sk, crp, noise, plaintext.value, [2]*ring.Poly{ciphertext.value[0], ciphertext.value[1]}, fast)
	ciphertext.isNTT = true
}
