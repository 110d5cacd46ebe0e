// Replacement body for github.com/ldsec/lattigo/bfv (v1.3.1), decryptor.go: this file is added to the package, the module's ring package
// is replaced by go/ring of this repository (INTEGRATION.md section 3), and the upstream body of the method defined here is DELETED from
// decryptor.go (same receiver and signature: Go has no virtual dispatch, see go/ckks/evaluator_device.go).
//
// NOT COMPILED IN THIS REPOSITORY'S PIPELINE (no Go toolchain in the image); statically checked by tests/test_go_bfv_encryptor.py.
//
// The patch to upstream bfv/decryptor.go, line numbers of v1.3.1:
//
//	delete  Decrypt  :55-75  -> below: ONE call, BfvDecryptor.Decrypt (the NTT of every component, Horner at the key with the
//	                            i&7 == 7 reduction cadence, InvNTT)
//	keep    NewDecryptor :28-45 (its polypool is no longer read), DecryptNew :47-53
package bfv

import (
	"sync"

	"github.com/ldsec/lattigo/ring"
)

var deviceDecryptors sync.Map // *decryptor -> *ring.BfvDecryptor

func (decryptor *decryptor) dev() *ring.BfvDecryptor {
	if d, ok := deviceDecryptors.Load(decryptor); ok {
		return d.(*ring.BfvDecryptor)
	}
	d := ring.NewBfvDecryptor(decryptor.bfvContext.contextQ, 1)
	actual, _ := deviceDecryptors.LoadOrStore(decryptor, d)
	return actual.(*ring.BfvDecryptor)
}

// ReleaseDevice drops the decryptor's device state and its entry in deviceDecryptors.
func (decryptor *decryptor) ReleaseDevice() {
	deviceDecryptors.Delete(decryptor)
}

// Decrypt (:55).
func (decryptor *decryptor) Decrypt(ciphertext *Ciphertext, plaintext *Plaintext) {
	decryptor.dev().Decrypt(ciphertext.value[:ciphertext.Degree()+1], decryptor.sk.sk, plaintext.value)
}
