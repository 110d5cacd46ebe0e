// Replacement bodies for github.com/ldsec/lattigo/dbfv (v1.3.1), public_refresh.go: this file is added to the package, the module's ring
// package is replaced by go/ring of this repository (INTEGRATION.md section 3), and the upstream bodies of the methods defined here are
// DELETED from public_refresh.go (same receivers and signatures: Go has no virtual dispatch, see go/ckks/evaluator_device.go).
//
// NOT COMPILED IN THIS REPOSITORY'S PIPELINE (no Go toolchain in the image); statically checked by tests/test_go_refresh.py.
//
// The patch to upstream dbfv/public_refresh.go, line numbers of v1.3.1:
//
//	delete  GenShares  :105-160  -> below: the two noises in compact form (KYSampler.SampleCompact), the mask uniform below t, then ONE
//	                                call, Refresh.BfvGenShares; lift (:199-205) runs inside it
//	delete  Aggregate  :163-166  -> below: Refresh.Aggregate per component
//	delete  Decrypt    :169-171  -> below: Refresh.Aggregate of ct[0] and the share (the Add)
//	delete  Finalize   :193-197  -> below: ONE call, Refresh.BfvFinalize
//	keep    NewRefreshProtocol :79-96, AllocateShares :99-102, Recode :174-179, Recrypt :182-190, RefreshShare.MarshalBinary :32-53,
//	        RefreshShare.UnmarshalBinary :56-76, lift and the struct: tmp1, tmp2 and hP stay allocated; Recode and Recrypt keep upstream's
//	        bodies for callers that run the steps one by one
//
// One deviation from upstream: rfp.hP is never zeroed there (cks.hP is, keyswitching.go:108), so a second GenShares on one RefreshProtocol
// accumulates unreduced noise; here every GenShares behaves as the first call on a fresh RefreshProtocol.  The noise comes from
// context.gaussianSampler where upstream makes a sampler with the same parameters per call (:113).
package dbfv

import (
	"crypto/rand"
	"math/big"
	"sync"

	"github.com/ldsec/lattigo/bfv"
	"github.com/ldsec/lattigo/ring"
)

var deviceRefreshProtocols sync.Map // *RefreshProtocol -> *ring.Refresh

func (rfp *RefreshProtocol) dev() *ring.Refresh {
	if r, ok := deviceRefreshProtocols.Load(rfp); ok {
		return r.(*ring.Refresh)
	}
	r := ring.NewRefresh(rfp.context.contextQ, rfp.context.contextP, rfp.context.params.T, 1)
	actual, _ := deviceRefreshProtocols.LoadOrStore(rfp, r)
	return actual.(*ring.Refresh)
}

// ReleaseDevice drops the protocol's device state and its entry in deviceRefreshProtocols.
func (rfp *RefreshProtocol) ReleaseDevice() {
	deviceRefreshProtocols.Delete(rfp)
}

// top is the level every BFV poly lives at.
func (rfp *RefreshProtocol) top() uint64 {
	return uint64(len(rfp.context.contextQ.Modulus) - 1)
}

// GenShares (:105).
func (rfp *RefreshProtocol) GenShares(sk *ring.Poly, ciphertext *bfv.Ciphertext, crs *ring.Poly, share RefreshShare) {
	e0 := make([]byte, rfp.context.n)
	e1 := make([]byte, rfp.context.n)
	rfp.context.gaussianSampler.SampleCompact(e0)
	rfp.context.gaussianSampler.SampleCompact(e1)
	t := new(big.Int).SetUint64(rfp.context.params.T)
	mask := make([]uint64, rfp.context.n)
	for i := range mask {
		m, err := rand.Int(rand.Reader, t)
		if err != nil {
			panic(err)
		}
		mask[i] = m.Uint64()
	}
	rfp.dev().BfvGenShares(sk, ciphertext.Value()[1], crs, mask, e0, e1, (*ring.Poly)(share.RefreshShareDecrypt), (*ring.Poly)(share.RefreshShareRecrypt))
}

// Aggregate (:163).
func (rfp *RefreshProtocol) Aggregate(share1, share2, shareOut RefreshShare) {
	rfp.dev().Aggregate(rfp.top(), []*ring.Poly{(*ring.Poly)(share1.RefreshShareDecrypt), (*ring.Poly)(share2.RefreshShareDecrypt)}, (*ring.Poly)(shareOut.RefreshShareDecrypt))
	rfp.dev().Aggregate(rfp.top(), []*ring.Poly{(*ring.Poly)(share1.RefreshShareRecrypt), (*ring.Poly)(share2.RefreshShareRecrypt)}, (*ring.Poly)(shareOut.RefreshShareRecrypt))
}

// Decrypt (:169).
func (rfp *RefreshProtocol) Decrypt(ciphertext *bfv.Ciphertext, shareDecrypt RefreshShareDecrypt, sharePlaintext *ring.Poly) {
	rfp.dev().Aggregate(rfp.top(), []*ring.Poly{ciphertext.Value()[0], (*ring.Poly)(shareDecrypt)}, sharePlaintext)
}

// Finalize (:193).
func (rfp *RefreshProtocol) Finalize(ciphertext *bfv.Ciphertext, crs *ring.Poly, share RefreshShare, ciphertextOut *bfv.Ciphertext) {
	rfp.dev().BfvFinalize(ciphertext.Value()[0], crs, (*ring.Poly)(share.RefreshShareDecrypt), (*ring.Poly)(share.RefreshShareRecrypt), ciphertextOut.Value()[0], ciphertextOut.Value()[1])
}
