// Replacement bodies for github.com/ldsec/lattigo/bfv (v1.3.1), encryptor.go: this file is added to the package, the module's ring package
// is replaced by go/ring of this repository (INTEGRATION.md section 3), and the upstream bodies of the methods defined here are DELETED
// from encryptor.go (same receivers and signatures: Go has no virtual dispatch, see go/ckks/evaluator_device.go).
//
// NOT COMPILED IN THIS REPOSITORY'S PIPELINE (no Go toolchain in the image); statically checked by tests/test_go_bfv_encryptor.py.
//
// The patch to upstream bfv/encryptor.go, line numbers of v1.3.1:
//
//	delete  pkEncryptor.encrypt  :169-223  -> below: the samplers' decisions in compact form (ring.SampleTernaryBits, KYSampler.SampleCompact
//	                                          twice, in upstream's order u, e0, e1), then ONE call, BfvEncryptor.EncryptPk.  In the fast
//	                                          branch upstream leaves the result in its pool; the device writes it to the ciphertext
//	delete  skEncryptor.encrypt  :306-345  -> below: the noise in compact form (KYSampler.SampleCompact, or the ziggurat of
//	                                          SampleGaussianAndAdd for the fast form), then ONE call, BfvEncryptor.EncryptSk; crp is read only
//	keep    newEncryptor :100-119, the Encrypt... wrappers :121-167, :225-284, encryptSample / encryptFromCRP :286-304 (they sample or copy
//	        the uniform poly into polypool[1] on the host and call encrypt)
package bfv

import (
	"sync"

	"github.com/ldsec/lattigo/ring"
)

var deviceEncryptors sync.Map // *encryptor -> *ring.BfvEncryptor

func (encryptor *encryptor) dev() *ring.BfvEncryptor {
	if e, ok := deviceEncryptors.Load(encryptor); ok {
		return e.(*ring.BfvEncryptor)
	}
	var contextP *ring.Context
	if encryptor.baseconverter != nil {
		contextP = encryptor.bfvContext.contextP
	}
	e := ring.NewBfvEncryptor(encryptor.bfvContext.contextQ, contextP, 1)
	actual, _ := deviceEncryptors.LoadOrStore(encryptor, e)
	return actual.(*ring.BfvEncryptor)
}

// ReleaseDevice drops the encryptor's device state and its entry in deviceEncryptors.
func (encryptor *encryptor) ReleaseDevice() {
	deviceEncryptors.Delete(encryptor)
}

// encrypt (:169).
func (encryptor *pkEncryptor) encrypt(plaintext *Plaintext, ciphertext *Ciphertext, fast bool) {
	n := len(plaintext.value.Coeffs[0])
	uCoeffs, uSigns := make([]byte, n>>3), make([]byte, n>>3)
	e0, e1 := make([]byte, n), make([]byte, n)
	ring.SampleTernaryBits(uCoeffs, uSigns)
	encryptor.bfvContext.gaussianSampler.SampleCompact(e0)
	encryptor.bfvContext.gaussianSampler.SampleCompact(e1)
	encryptor.dev().EncryptPk(encryptor.pk.pk, uCoeffs, uSigns, e0, e1, plaintext.value, [2]*ring.Poly{ciphertext.value[0], ciphertext.value[1]}, fast)
}

// encrypt (:306).
func (encryptor *skEncryptor) encrypt(plaintext *Plaintext, ciphertext *Ciphertext, crp *ring.Poly, fast bool) {
	noise := make([]byte, len(plaintext.value.Coeffs[0]))
	if fast {
		encryptor.bfvContext.contextQ.SampleGaussianCompact(noise, encryptor.params.Sigma, uint64(6*encryptor.params.Sigma))
	} else {
		encryptor.bfvContext.gaussianSampler.SampleCompact(noise)
	}
	encryptor.dev().EncryptSk(encryptor.sk.sk, crp, noise, plaintext.value, [2]*ring.Poly{ciphertext.value[0], ciphertext.value[1]}, fast)
}
