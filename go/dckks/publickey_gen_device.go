// Replacement bodies for github.com/ldsec/lattigo/dckks (v1.3.1), publickey_gen.go: this file is added to the package, the module's ring package
// is replaced by go/ring of this repository (INTEGRATION.md section 3), and the upstream bodies of the methods defined here are DELETED
// from publickey_gen.go (same receivers and signatures: Go has no virtual dispatch, see go/ckks/evaluator_device.go).
//
// NOT COMPILED IN THIS REPOSITORY'S PIPELINE (no Go toolchain in the image); statically checked by tests/test_go_setup.py.
//
// The patch to upstream dckks/publickey_gen.go, line numbers of v1.3.1:
//
//	delete  GenShare         :39-42    -> below: the noise in compact form (KYSampler.SampleCompact), then ONE call, Setup.CkgShare,
//	                                      on contextQP taken as a ring without P: every row alike
//	delete  AggregateShares  :45-47    -> below: Setup.Aggregate over the two shares
//	keep    NewCKGProtocol :18-27, AllocateShares :30-32, GenPublicKey :50-52 (a Set) and the struct
package dckks

import (
	"sync"

	"github.com/ldsec/lattigo/ring"
)

var deviceCKGProtocols sync.Map // *CKGProtocol -> *ring.Setup

func (ckg *CKGProtocol) dev() *ring.Setup {
	if s, ok := deviceCKGProtocols.Load(ckg); ok {
		return s.(*ring.Setup)
	}
	s := ring.NewSetup(ckg.dckksContext.contextQP, nil, 1)
	actual, _ := deviceCKGProtocols.LoadOrStore(ckg, s)
	return actual.(*ring.Setup)
}

// ReleaseDevice drops the protocol's device state and its entry in deviceCKGProtocols.
func (ckg *CKGProtocol) ReleaseDevice() {
	deviceCKGProtocols.Delete(ckg)
}

// GenShare (:39).
func (ckg *CKGProtocol) GenShare(sk *ring.Poly, crs *ring.Poly, shareOut CKGShare) {
	noise := make([]byte, ckg.dckksContext.n)
	ckg.dckksContext.gaussianSampler.SampleCompact(noise)
	ckg.dev().CkgShare(sk, crs, noise, shareOut)
}

// AggregateShares (:45).
func (ckg *CKGProtocol) AggregateShares(share1, share2, shareOut CKGShare) {
	ckg.dev().Aggregate([]*ring.Poly{share1, share2}, shareOut)
}
