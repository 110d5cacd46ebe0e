// Replacement bodies for github.com/ldsec/lattigo/dckks (v1.3.1), public_keyswitching.go: this file is added to the package, the module's ring package
// is replaced by go/ring of this repository (INTEGRATION.md section 3), and the upstream bodies of the methods defined here are DELETED
// from public_keyswitching.go (same receivers and signatures: Go has no virtual dispatch, see go/ckks/evaluator_device.go).
//
// NOT COMPILED IN THIS REPOSITORY'S PIPELINE (no Go toolchain in the image); statically checked by tests/test_go_collective.py.
//
// The patch to upstream dckks/public_keyswitching.go, line numbers of v1.3.1:
//
//	delete  GenShare         :63-93    -> below: the samplers' decisions in compact form in upstream's order -- u (ring.SampleTernaryBits), e0 from
//	                                      the smudging sampler, e1 from the regular one (KYSampler.SampleCompact) -- then ONE call,
//	                                      Collective.CkksPcksShare at ct.Level()
//	delete  AggregateShares  :99-104   -> below: Collective.Aggregate per component
//	delete  KeySwitch        :107-113  -> below: Collective.Aggregate with ct[0] as the base (the Add), then with combined[1] alone (the Copy)
//	keep    NewPCKSProtocol :28-49, AllocateShares :52-56 and the struct: tmp, share0tmp and share1tmp stay allocated and unused
package dckks

import (
	"sync"

	"github.com/ldsec/lattigo/ckks"
	"github.com/ldsec/lattigo/ring"
)

var devicePCKSProtocols sync.Map // *PCKSProtocol -> *ring.Collective

func (pcks *PCKSProtocol) dev() *ring.Collective {
	if c, ok := devicePCKSProtocols.Load(pcks); ok {
		return c.(*ring.Collective)
	}
	c := ring.NewCollective(pcks.dckksContext.contextQ, pcks.dckksContext.contextP, 1)
	actual, _ := devicePCKSProtocols.LoadOrStore(pcks, c)
	return actual.(*ring.Collective)
}

// ReleaseDevice drops the protocol's device state and its entry in devicePCKSProtocols.
func (pcks *PCKSProtocol) ReleaseDevice() {
	devicePCKSProtocols.Delete(pcks)
}

// GenShare (:63).
func (pcks *PCKSProtocol) GenShare(sk *ring.Poly, pk *ckks.PublicKey, ct *ckks.Ciphertext, shareOut PCKSShare) {
	n := pcks.dckksContext.n
	uCoeffs, uSigns := make([]byte, n>>3), make([]byte, n>>3)
	e0, e1 := make([]byte, n), make([]byte, n)
	ring.SampleTernaryBits(uCoeffs, uSigns)
	pcks.gaussianSamplerSmudge.SampleCompact(e0)
	pcks.dckksContext.gaussianSampler.SampleCompact(e1)
	pcks.dev().CkksPcksShare(ct.Level(), sk, pk.Get(), ct.Value()[1], uCoeffs, uSigns, e0, e1, shareOut)
}

// AggregateShares (:99).
func (pcks *PCKSProtocol) AggregateShares(share1, share2, shareOut PCKSShare) {
	level := uint64(len(share1[0].Coeffs)) - 1
	pcks.dev().Aggregate(level, nil, []*ring.Poly{share1[0], share2[0]}, shareOut[0])
	pcks.dev().Aggregate(level, nil, []*ring.Poly{share1[1], share2[1]}, shareOut[1])
}

// KeySwitch (:107).
func (pcks *PCKSProtocol) KeySwitch(combined PCKSShare, ct, ctOut *ckks.Ciphertext) {
	ctOut.SetScale(ct.Scale())
	pcks.dev().Aggregate(ct.Level(), ct.Value()[0], []*ring.Poly{combined[0]}, ctOut.Value()[0])
	pcks.dev().Aggregate(ct.Level(), nil, []*ring.Poly{combined[1]}, ctOut.Value()[1])
}
