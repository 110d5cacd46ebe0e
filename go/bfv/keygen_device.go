// Replacement bodies for github.com/ldsec/lattigo/bfv (v1.3.1), keygen.go: this file is added to the package, the module's ring package is
// replaced by go/ring of this repository (INTEGRATION.md section 3), and the upstream bodies of the methods defined here are DELETED from
// keygen.go (same receivers and signatures: Go has no virtual dispatch, see go/bfv/evaluator_device.go).
//
// NOT COMPILED IN THIS REPOSITORY'S PIPELINE (no Go toolchain in the image); statically checked by tests/test_go_keygen.py.
//
// The patch to upstream bfv/keygen.go, line numbers of v1.3.1:
//
//	delete  GenPublicKey         :121-136  -> below: the noise in compact form (KYSampler.SampleCompact), the uniform poly as upstream
//	                                          draws it, then ONE call, KeyGenerator.GenPublicKey
//	delete  GenRelinKey          :172-196  -> below: ONE call, KeyGenerator.GenRelinKeys, makes the maxDegree keys (the running product
//	                                          with sk runs on the device)
//	delete  GenSwitchingKey      :247-261  -> below: KeyGenerator.GenSwitchingKeys on skIn as it is
//	delete  newswitchingkey      :285-333  (no caller left: upstream hands it P skIn, the device multiplies by P itself -- the two
//	                                          orders give the same bits, tests/test_oracle_keygen.py)
//	delete  GenRot               :342-368  -> below: upstream's bookkeeping around genrotkey
//	delete  GenRotationKeysPow2  :372-388  -> below: the samplers run per key and digit in upstream's order, then ONE call,
//	                                          KeyGenerator.GenRotationKeys, makes all 2 (logN - 1) + 1 keys
//	delete  genrotkey            :429-441  -> below: KeyGenerator.GenRotationKeys with one Galois element
//	keep    GenSecretKey, GenSecretkeyWithDistrib :87-96 (the ternary sampler of ring stays on the host: it consumes crypto/rand
//	        serially), GenKeyPair :165-168, every New..., Get and Set
//
// Every generated SwitchingKey is registered with its device image in generatedKeyImages: evaluator.keyImage
// (go/bfv/evaluator_device.go) finds it there, takes it over and uploads nothing; ReleaseGeneratedKey drops one no evaluator took.  DeviceKeysHostCopy = false leaves evakey[i][0] zero on the host.
package bfv

import (
	"sync"

	"github.com/ldsec/lattigo/ring"
)

var deviceKeyGenerators sync.Map // *keyGenerator -> *ring.KeyGenerator
var generatedKeyImages sync.Map  // *SwitchingKey -> *ring.Poly

// DeviceKeysHostCopy: download evakey[i][0] after the generation, so that marshalling and Set... see the key on the host.
var DeviceKeysHostCopy = true

func (keygen *keyGenerator) dev() *ring.KeyGenerator {
	if g, ok := deviceKeyGenerators.Load(keygen); ok {
		return g.(*ring.KeyGenerator)
	}
	maxKeys := 2*int(keygen.params.LogN) - 1 // GenRotationKeysPow2's set in one call
	g := ring.NewKeyGenerator(keygen.bfvContext.contextQ, keygen.bfvContext.contextP, maxKeys)
	actual, _ := deviceKeyGenerators.LoadOrStore(keygen, g)
	return actual.(*ring.KeyGenerator)
}

// ReleaseGeneratedKey drops the device image of a generated key that no evaluator has taken yet (a key made only to be marshalled):
// the image's finalizer then frees its device memory.  An evaluator's first use of a key moves the image out of generatedKeyImages
// into its own state, which evaluator.ReleaseDevice lets go; a second evaluator uploads the key from the host copy.
func ReleaseGeneratedKey(k *SwitchingKey) {
	generatedKeyImages.Delete(k)
}

// ReleaseDevice drops the key generator's device state and its entry in deviceKeyGenerators.
func (keygen *keyGenerator) ReleaseDevice() {
	deviceKeyGenerators.Delete(keygen)
}

// sampleKey draws what newswitchingkey draws for one key, per digit in upstream's order (:301, :304): the noise in compact form, appended
// to noise, and the uniform poly into evakey[i][1]; evakey[i][0] is allocated.
func (keygen *keyGenerator) sampleKey(noise []byte) (*SwitchingKey, []byte) {
	ringContext := keygen.bfvContext.contextQP
	k := new(SwitchingKey)
	k.evakey = make([][2]*ring.Poly, keygen.params.beta)
	for i := uint64(0); i < keygen.params.beta; i++ {
		e := make([]byte, ringContext.N)
		keygen.bfvContext.gaussianSampler.SampleCompact(e)
		noise = append(noise, e...)
		k.evakey[i][0] = ringContext.NewPoly()
		k.evakey[i][1] = ringContext.NewUniformPoly()
	}
	return k, noise
}

func (keygen *keyGenerator) image(k *SwitchingKey) *ring.Poly {
	uniform := make([]*ring.Poly, len(k.evakey))
	for i := range k.evakey {
		uniform[i] = k.evakey[i][1]
	}
	return keygen.dev().NewSwitchingKeyImage(uniform)
}

func (keygen *keyGenerator) finish(k *SwitchingKey, img *ring.Poly) {
	generatedKeyImages.Store(k, img)
	if DeviceKeysHostCopy {
		keygen.dev().DownloadKey(img, k.evakey)
	}
}

// GenPublicKey (:121).
func (keygen *keyGenerator) GenPublicKey(sk *SecretKey) (pk *PublicKey) {
	pk = new(PublicKey)
	ringContext := keygen.bfvContext.contextQP
	noise := make([]byte, ringContext.N)
	keygen.bfvContext.gaussianSampler.SampleCompact(noise)
	pk.pk[0] = ringContext.NewPoly()
	pk.pk[1] = ringContext.NewUniformPoly()
	keygen.dev().GenPublicKey(sk.sk, noise, pk.pk)
	return pk
}

// GenRelinKey (:172).
func (keygen *keyGenerator) GenRelinKey(sk *SecretKey, maxDegree uint64) (evk *EvaluationKey) {
	if keygen.bfvContext.contextP == nil {
		panic("Cannot GenRelinKey: modulus P is empty")
	}
	evk = new(EvaluationKey)
	evk.evakey = make([]*SwitchingKey, maxDegree)
	var noise []byte
	images := make([]*ring.Poly, maxDegree)
	for i := uint64(0); i < maxDegree; i++ {
		evk.evakey[i], noise = keygen.sampleKey(noise)
		images[i] = keygen.image(evk.evakey[i])
	}
	keygen.dev().GenRelinKeys(sk.Get(), noise, images)
	for i := range images {
		keygen.finish(evk.evakey[i], images[i])
	}
	return
}

// GenSwitchingKey (:247).
func (keygen *keyGenerator) GenSwitchingKey(skIn, skOut *SecretKey) (evk *SwitchingKey) {
	if keygen.bfvContext.contextP == nil {
		panic("Cannot GenRelinKey: modulus P is empty")
	}
	evk, noise := keygen.sampleKey(nil)
	img := keygen.image(evk)
	keygen.dev().GenSwitchingKeys(skIn.Get(), skOut.Get(), noise, []*ring.Poly{img})
	keygen.finish(evk, img)
	return
}

// genrotkey (:429).
func genrotkey(keygen *keyGenerator, sk *ring.Poly, gen uint64) (switchkey *SwitchingKey) {
	switchkey, noise := keygen.sampleKey(nil)
	img := keygen.image(switchkey)
	keygen.dev().GenRotationKeys(sk, []uint64{gen}, noise, []*ring.Poly{img})
	keygen.finish(switchkey, img)
	return
}

// GenRot (:342).
func (keygen *keyGenerator) GenRot(rotType Rotation, sk *SecretKey, k uint64, rotKey *RotationKeys) {
	if keygen.bfvContext.contextP == nil {
		panic("Cannot GenRelinKey: modulus P is empty")
	}
	k &= ((keygen.bfvContext.n >> 1) - 1)
	switch rotType {
	case RotationLeft:
		if rotKey.evakeyRotColLeft == nil {
			rotKey.evakeyRotColLeft = make(map[uint64]*SwitchingKey)
		}
		if rotKey.evakeyRotColLeft[k] == nil && k != 0 {
			rotKey.evakeyRotColLeft[k] = genrotkey(keygen, sk.Get(), keygen.bfvContext.galElRotColLeft[k])
		}
	case RotationRight:
		if rotKey.evakeyRotColRight == nil {
			rotKey.evakeyRotColRight = make(map[uint64]*SwitchingKey)
		}
		if rotKey.evakeyRotColRight[k] == nil && k != 0 {
			rotKey.evakeyRotColRight[k] = genrotkey(keygen, sk.Get(), keygen.bfvContext.galElRotColRight[k])
		}
	case RotationRow:
		rotKey.evakeyRotRow = genrotkey(keygen, sk.Get(), keygen.bfvContext.galElRotRow)
	}
}

// GenRotationKeysPow2 (:372).
func (keygen *keyGenerator) GenRotationKeysPow2(sk *SecretKey) (rotKey *RotationKeys) {
	rotKey = new(RotationKeys)
	rotKey.evakeyRotColLeft = make(map[uint64]*SwitchingKey)
	rotKey.evakeyRotColRight = make(map[uint64]*SwitchingKey)
	var noise []byte
	var keys []*SwitchingKey
	var images []*ring.Poly
	var galEls []uint64
	add := func(gen uint64) *SwitchingKey {
		var k *SwitchingKey
		k, noise = keygen.sampleKey(noise)
		keys, images, galEls = append(keys, k), append(images, keygen.image(k)), append(galEls, gen)
		return k
	}
	for n := uint64(1); n < keygen.bfvContext.n>>1; n <<= 1 {
		rotKey.evakeyRotColLeft[n] = add(keygen.bfvContext.galElRotColLeft[n])
		rotKey.evakeyRotColRight[n] = add(keygen.bfvContext.galElRotColRight[n])
	}
	rotKey.evakeyRotRow = add(keygen.bfvContext.galElRotRow)
	keygen.dev().GenRotationKeys(sk.Get(), galEls, noise, images)
	for i, k := range keys {
		keygen.finish(k, images[i])
	}
	return
}
