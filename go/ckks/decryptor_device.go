// Replacement body for github.com/ldsec/lattigo/ckks (v1.3.1), decryptor.go: this file is added to the package, the module's ring package
// is replaced by go/ring of this repository (INTEGRATION.md section 3), and the upstream body of the method defined here is DELETED from
// decryptor.go (same receiver and signature: Go has no virtual dispatch, see go/ckks/evaluator_device.go).
//
// NOT COMPILED IN THIS REPOSITORY'S PIPELINE (no Go toolchain in the image); statically checked by tests/test_go_ckks_encryptor.py.
//
// The patch to upstream ckks/decryptor.go, line numbers of v1.3.1:
//
//	delete  Decrypt  :53-78  -> below: upstream's scale and limb bookkeeping, then ONE call, CkksPlan.Decrypt (Horner at the key with the
//	                            i&7 == 7 reduction cadence, every operand read once)
//	keep    NewDecryptor :24-38, DecryptNew :42-49 (it calls Decrypt)
package ckks

import (
	"sync"

	"github.com/ldsec/lattigo/ring"
)

var deviceCkksDecryptors sync.Map // *decryptor -> *ring.CkksPlan

func (decryptor *decryptor) dev() *ring.CkksPlan {
	if d, ok := deviceCkksDecryptors.Load(decryptor); ok {
		return d.(*ring.CkksPlan)
	}
	d := ring.NewCkksPlan(decryptor.ckksContext.contextQ, decryptor.ckksContext.contextP, 1)
	actual, _ := deviceCkksDecryptors.LoadOrStore(decryptor, d)
	return actual.(*ring.CkksPlan)
}

// ReleaseDevice drops the decryptor's device state and its entry in deviceCkksDecryptors.
func (decryptor *decryptor) ReleaseDevice() {
	deviceCkksDecryptors.Delete(decryptor)
}

// Decrypt (:53).
func (decryptor *decryptor) Decrypt(ciphertext *Ciphertext, plaintext *Plaintext) {
	level := ciphertext.Level()
	plaintext.SetScale(ciphertext.Scale())
	plaintext.value.Coeffs = plaintext.value.Coeffs[:level+1]
	decryptor.dev().Decrypt(level, ciphertext.value[:ciphertext.Degree()+1], decryptor.sk.sk, plaintext.value)
}
