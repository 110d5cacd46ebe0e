// Replacement bodies for github.com/ldsec/lattigo/dbfv (v1.3.1), rotkey_gen.go: this file is added to the package, the module's ring package
// is replaced by go/ring of this repository (INTEGRATION.md section 3), and the upstream bodies of the methods defined here are DELETED
// from rotkey_gen.go (same receivers and signatures: Go has no virtual dispatch, see go/ckks/evaluator_device.go).
//
// NOT COMPILED IN THIS REPOSITORY'S PIPELINE (no Go toolchain in the image); statically checked by tests/test_go_setup.py.
//
// The patch to upstream dbfv/rotkey_gen.go, line numbers of v1.3.1:
//
//	delete  genShare   :139  -> below: beta noise polys in compact form, then ONE call, Setup.RtgShare (the Galois gather of sk, the
//	                            digit add, the product with crp and the MForm in one pass); tmpPoly unused
//	delete  Aggregate  :190  -> below: the same checks, then Setup.Aggregate over two images of beta polys
//	delete  Finalize   :205  -> below: Setup.RtgKey into a key image, downloaded into tmpSwitchKey for SetRotKey
//	keep    NewRotKGProtocol, AllocateShare, GenShare (the map from (rotation type, k) to a Galois element), the two marshalers and the struct
package dbfv

import (
	"sync"

	"github.com/ldsec/lattigo/bfv"
	"github.com/ldsec/lattigo/ring"
)

var deviceRTGProtocols sync.Map // *RTGProtocol -> *ring.Setup

func (rtg *RTGProtocol) dev() *ring.Setup {
	if s, ok := deviceRTGProtocols.Load(rtg); ok {
		return s.(*ring.Setup)
	}
	s := ring.NewSetup(rtg.context.contextQ, rtg.context.contextP, 1)
	actual, _ := deviceRTGProtocols.LoadOrStore(rtg, s)
	return actual.(*ring.Setup)
}

// ReleaseDevice drops the protocol's device state and its entry in deviceRTGProtocols.
func (rtg *RTGProtocol) ReleaseDevice() {
	deviceRTGProtocols.Delete(rtg)
}

// genShare (:139).
func (rtg *RTGProtocol) genShare(sk *ring.Poly, galEl uint64, crp []*ring.Poly, evakey []*ring.Poly) {
	beta := rtg.context.params.Beta()
	n := rtg.context.n
	noise := make([]byte, beta*n)
	for i := uint64(0); i < beta; i++ {
		rtg.context.gaussianSampler.SampleCompact(noise[i*n : (i+1)*n])
	}
	d := rtg.dev()
	out := d.NewImage(int(beta))
	d.RtgShare(sk, []uint64{galEl}, d.ShareImage(crp), noise, []*ring.Poly{out})
	d.DownloadShare(out, evakey)
}

// Aggregate (:190).
func (rtg *RTGProtocol) Aggregate(share1, share2, shareOut RTGShare) {
	if share1.Type != share2.Type || share1.K != share2.K {
		panic("cannot aggregate shares of different types")
	}
	shareOut.Type = share1.Type
	shareOut.K = share1.K
	d := rtg.dev()
	out := d.NewImage(len(shareOut.Value))
	d.Aggregate([]*ring.Poly{d.ShareImage(share1.Value), d.ShareImage(share2.Value)}, out)
	d.DownloadShare(out, shareOut.Value)
}

// Finalize (:205).
func (rtg *RTGProtocol) Finalize(share RTGShare, crp []*ring.Poly, rotKey *bfv.RotationKeys) {
	k := share.K & ((rtg.context.n >> 1) - 1)
	d := rtg.dev()
	key := d.NewImage(2 * len(share.Value))
	d.RtgKey(d.ShareImage(share.Value), d.ShareImage(crp), key)
	d.DownloadPairs(key, rtg.tmpSwitchKey)
	rotKey.SetRotKey(share.Type, k, rtg.tmpSwitchKey)
}
