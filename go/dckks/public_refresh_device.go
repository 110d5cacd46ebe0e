// Replacement bodies for github.com/ldsec/lattigo/dckks (v1.3.1), public_refresh.go: this file is added to the package, the module's ring
// package is replaced by go/ring of this repository (INTEGRATION.md section 3), and the upstream bodies of the methods defined here are
// DELETED from public_refresh.go (same receivers and signatures: Go has no virtual dispatch, see go/ckks/evaluator_device.go).
//
// NOT COMPILED IN THIS REPOSITORY'S PIPELINE (no Go toolchain in the image); statically checked by tests/test_go_refresh.py.
//
// The patch to upstream dckks/public_refresh.go, line numbers of v1.3.1:
//
//	delete  GenShares  :43-95    -> below: the masks drawn below Q_levelStart / 2n and centred as upstream draws them, packed into word
//	                                planes (ring.MaskWordPlanes), the two noises in compact form (KYSampler.SampleCompact), then ONE call,
//	                                Refresh.CkksGenShares; the masks are zeroed afterwards as at :70-72
//	delete  Aggregate  :98-100   -> below: Refresh.Aggregate over the two shares
//	delete  Decrypt    :103-105  -> below: Refresh.Aggregate of ct[0] and the share onto ct[0] (the AddLvl)
//	delete  Recode     :108-139  -> below: Refresh.CkksRecode into a poly over all of Q that becomes ct[0]
//	delete  Recrypt    :142-147  -> below: Refresh.Aggregate of ct[0] and the share over all of Q, then ct[1] = crs.CopyNew()
//	keep    NewRefreshProtocol :23-35, AllocateShares :38-40 and the struct: tmp stays allocated and unused
//
// The noise comes from dckksContext.gaussianSampler where upstream makes a sampler with the same parameters per call (:46).
package dckks

import (
	"crypto/rand"
	"math/big"
	"sync"

	"github.com/ldsec/lattigo/ckks"
	"github.com/ldsec/lattigo/ring"
)

var deviceRefreshProtocols sync.Map // *RefreshProtocol -> *ring.Refresh

func (refreshProtocol *RefreshProtocol) dev() *ring.Refresh {
	if r, ok := deviceRefreshProtocols.Load(refreshProtocol); ok {
		return r.(*ring.Refresh)
	}
	r := ring.NewRefresh(refreshProtocol.dckksContext.contextQ, nil, 0, 1)
	actual, _ := deviceRefreshProtocols.LoadOrStore(refreshProtocol, r)
	return actual.(*ring.Refresh)
}

// ReleaseDevice drops the protocol's device state and its entry in deviceRefreshProtocols.
func (refreshProtocol *RefreshProtocol) ReleaseDevice() {
	deviceRefreshProtocols.Delete(refreshProtocol)
}

// top is the level of a refreshed ciphertext.
func (refreshProtocol *RefreshProtocol) top() uint64 {
	return uint64(len(refreshProtocol.dckksContext.contextQ.Modulus) - 1)
}

// GenShares (:43).
func (refreshProtocol *RefreshProtocol) GenShares(sk *ring.Poly, levelStart, nParties uint64, ciphertext *ckks.Ciphertext, crs *ring.Poly, shareDecrypt RefreshShareDecrypt, shareRecrypt RefreshShareRecrypt) {
	context := refreshProtocol.dckksContext.contextQ
	bound := big.NewInt(1)
	for i := uint64(0); i < levelStart+1; i++ {
		bound.Mul(bound, new(big.Int).SetUint64(context.Modulus[i]))
	}
	bound.Quo(bound, new(big.Int).SetUint64(2*nParties))
	half := new(big.Int).Rsh(bound, 1)
	for i := range refreshProtocol.maskBigint {
		m, err := rand.Int(rand.Reader, bound)
		if err != nil {
			panic(err)
		}
		if m.Cmp(half) >= 0 {
			m.Sub(m, bound)
		}
		refreshProtocol.maskBigint[i] = m
	}
	planes := ring.MaskWordPlanes(refreshProtocol.maskBigint, refreshProtocol.dev().MaskWords(levelStart))
	for i := range refreshProtocol.maskBigint {
		refreshProtocol.maskBigint[i] = new(big.Int)
	}
	e0 := make([]byte, refreshProtocol.dckksContext.n)
	e1 := make([]byte, refreshProtocol.dckksContext.n)
	refreshProtocol.dckksContext.gaussianSampler.SampleCompact(e0)
	refreshProtocol.dckksContext.gaussianSampler.SampleCompact(e1)
	refreshProtocol.dev().CkksGenShares(sk, levelStart, ciphertext.Value()[1], crs, planes, e0, e1, (*ring.Poly)(shareDecrypt), (*ring.Poly)(shareRecrypt))
}

// Aggregate (:98).
func (refreshProtocol *RefreshProtocol) Aggregate(share1, share2, shareOut *ring.Poly) {
	refreshProtocol.dev().Aggregate(uint64(len(share1.Coeffs)-1), []*ring.Poly{share1, share2}, shareOut)
}

// Decrypt (:103).
func (refreshProtocol *RefreshProtocol) Decrypt(ciphertext *ckks.Ciphertext, shareDecrypt RefreshShareDecrypt) {
	refreshProtocol.dev().Aggregate(ciphertext.Level(), []*ring.Poly{ciphertext.Value()[0], (*ring.Poly)(shareDecrypt)}, ciphertext.Value()[0])
}

// Recode (:108).
func (refreshProtocol *RefreshProtocol) Recode(ciphertext *ckks.Ciphertext) {
	out := refreshProtocol.dckksContext.contextQ.NewPoly()
	refreshProtocol.dev().CkksRecode(ciphertext.Level(), ciphertext.Value()[0], out)
	ciphertext.Value()[0] = out
}

// Recrypt (:142).
func (refreshProtocol *RefreshProtocol) Recrypt(ciphertext *ckks.Ciphertext, crs *ring.Poly, shareRecrypt RefreshShareRecrypt) {
	refreshProtocol.dev().Aggregate(refreshProtocol.top(), []*ring.Poly{ciphertext.Value()[0], (*ring.Poly)(shareRecrypt)}, ciphertext.Value()[0])
	ciphertext.Value()[1] = crs.CopyNew()
}
