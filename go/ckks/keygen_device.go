// Replacement bodies for github.com/ldsec/lattigo/ckks (v1.3.1), keygen.go: this file is added to the package, the module's ring package
// is replaced by go/ring of this repository (INTEGRATION.md section 3), and the upstream bodies of the methods defined here are DELETED
// from keygen.go (same receivers and signatures: Go has no virtual dispatch, see go/ckks/evaluator_device.go).
//
// NOT COMPILED IN THIS REPOSITORY'S PIPELINE (no Go toolchain in the image); statically checked by tests/test_go_keygen.py.
//
// The patch to upstream ckks/keygen.go, line numbers of v1.3.1:
//
//	delete  GenPublicKey         :138-151  -> below: the noise in compact form (KYSampler.SampleCompact), the uniform poly as upstream
//	                                          draws it, then ONE call, KeyGenerator.GenPublicKey
//	delete  GenRelinKey          :192-205  -> below: KeyGenerator.GenRelinKeys with one image (the product sk sk runs on the device)
//	delete  GenSwitchingKey      :247-258  -> below: newSwitchingKey on skInput as it is
//	delete  newSwitchingKey      :282-338  -> below: per digit, in upstream's order, the noise in compact form and the uniform poly; then
//	                                          ONE call, KeyGenerator.GenSwitchingKeys (the multiplication by P, MForm, the digit's Add
//	                                          and MulCoeffsMontgomeryAndSub run on the device); skIn is NOT modified (upstream multiplies
//	                                          its pool poly by P in place and zeroes it afterwards)
//	delete  GenRot               :347-388  -> below: upstream's bookkeeping around genrotKey
//	delete  GenRotationKeysPow2  :391-417  -> below: the samplers run per key and digit in upstream's order, then ONE call,
//	                                          KeyGenerator.GenRotationKeys, makes all 2 (logN - 1) + 1 keys
//	delete  genrotKey            :487-494  -> below: KeyGenerator.GenRotationKeys with one Galois element (PermuteNTT runs on the device)
//	keep    GenSecretKey, GenSecretKeyWithDistrib, GenSecretKeySparse :97-113 (the ternary samplers of ring stay on the host: they
//	        consume crypto/rand serially), GenKeyPair, GenKeyPairSparse :180-189, every New..., Get and Set
//
// Every generated SwitchingKey is registered with its device image in generatedKeyImages: evaluator.keyImage
// (go/ckks/evaluator_device.go) finds it there, takes it over and uploads nothing; ReleaseGeneratedKey drops one no evaluator took.  DeviceKeysHostCopy = false leaves evakey[i][0] zero on the host
// (keys that are only ever used by evaluators of this process).
package ckks

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
	g := ring.NewKeyGenerator(keygen.ckksContext.contextQ, keygen.ckksContext.contextP, maxKeys)
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

// sampleKey draws what newSwitchingKey draws for one key, per digit in upstream's order (:302, :306): the noise in compact form, appended
// to noise, and the uniform poly into evakey[i][1]; evakey[i][0] is allocated.
func (keygen *keyGenerator) sampleKey(noise []byte) (*SwitchingKey, []byte) {
	beta := keygen.params.Beta()
	n := keygen.ringContext.N
	k := new(SwitchingKey)
	k.evakey = make([][2]*ring.Poly, beta)
	for i := uint64(0); i < beta; i++ {
		e := make([]byte, n)
		keygen.ckksContext.gaussianSampler.SampleCompact(e)
		noise = append(noise, e...)
		k.evakey[i][0] = keygen.ringContext.NewPoly()
		k.evakey[i][1] = keygen.ringContext.NewUniformPoly()
	}
	return k, noise
}

// image builds the device image of a sampled key; finish registers it and copies the generated half to the host.
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

// GenPublicKey (:138).
func (keygen *keyGenerator) GenPublicKey(sk *SecretKey) (pk *PublicKey) {
	pk = new(PublicKey)
	noise := make([]byte, keygen.ringContext.N)
	keygen.ckksContext.gaussianSampler.SampleCompact(noise)
	pk.pk[0] = keygen.ringContext.NewPoly()
	pk.pk[1] = keygen.ringContext.NewUniformPoly()
	keygen.dev().GenPublicKey(sk.sk, noise, pk.pk)
	return pk
}

// GenRelinKey (:192).
func (keygen *keyGenerator) GenRelinKey(sk *SecretKey) (evakey *EvaluationKey) {
	if keygen.ckksContext.contextP == nil {
		panic("Cannot GenRelinKey: modulus P is empty")
	}
	evakey = new(EvaluationKey)
	k, noise := keygen.sampleKey(nil)
	img := keygen.image(k)
	keygen.dev().GenRelinKeys(sk.sk, noise, []*ring.Poly{img})
	keygen.finish(k, img)
	evakey.evakey = k
	return
}

// GenSwitchingKey (:247).
func (keygen *keyGenerator) GenSwitchingKey(skInput, skOutput *SecretKey) (newevakey *SwitchingKey) {
	if keygen.ckksContext.contextP == nil {
		panic("Cannot GenSwitchingKey: modulus P is empty")
	}
	return keygen.newSwitchingKey(skInput.sk, skOutput.sk)
}

// newSwitchingKey (:282).
func (keygen *keyGenerator) newSwitchingKey(skIn, skOut *ring.Poly) (switchingkey *SwitchingKey) {
	switchingkey, noise := keygen.sampleKey(nil)
	img := keygen.image(switchingkey)
	keygen.dev().GenSwitchingKeys(skIn, skOut, noise, []*ring.Poly{img})
	keygen.finish(switchingkey, img)
	return
}

// genrotKey (:487).
func (keygen *keyGenerator) genrotKey(skOutput *ring.Poly, gen uint64) (switchingkey *SwitchingKey) {
	switchingkey, noise := keygen.sampleKey(nil)
	img := keygen.image(switchingkey)
	keygen.dev().GenRotationKeys(skOutput, []uint64{gen}, noise, []*ring.Poly{img})
	keygen.finish(switchingkey, img)
	return
}

// GenRot (:347).
func (keygen *keyGenerator) GenRot(rotType Rotation, sk *SecretKey, k uint64, rotKey *RotationKeys) {
	if keygen.ckksContext.contextP == nil {
		panic("Cannot GenRot: modulus P is empty")
	}
	switch rotType {
	case RotationLeft:
		if rotKey.evakeyRotColLeft == nil {
			rotKey.evakeyRotColLeft = make(map[uint64]*SwitchingKey)
		}
		if rotKey.permuteNTTLeftIndex == nil {
			rotKey.permuteNTTLeftIndex = make(map[uint64][]uint64)
		}
		if rotKey.evakeyRotColLeft[k] == nil && k != 0 {
			rotKey.permuteNTTLeftIndex[k] = ring.PermuteNTTIndex(GaloisGen, k, keygen.ringContext.N)
			rotKey.evakeyRotColLeft[k] = keygen.genrotKey(sk.Get(), keygen.ckksContext.galElRotColLeft[k])
		}
	case RotationRight:
		if rotKey.evakeyRotColRight == nil {
			rotKey.evakeyRotColRight = make(map[uint64]*SwitchingKey)
		}
		if rotKey.permuteNTTRightIndex == nil {
			rotKey.permuteNTTRightIndex = make(map[uint64][]uint64)
		}
		if rotKey.evakeyRotColRight[k] == nil && k != 0 {
			rotKey.permuteNTTRightIndex[k] = ring.PermuteNTTIndex(GaloisGen, 2*keygen.ringContext.N-k, keygen.ringContext.N)
			rotKey.evakeyRotColRight[k] = keygen.genrotKey(sk.Get(), keygen.ckksContext.galElRotColRight[k])
		}
	case Conjugate:
		rotKey.permuteNTTConjugateIndex = ring.PermuteNTTIndex(2*keygen.ringContext.N-1, 1, keygen.ringContext.N)
		rotKey.evakeyConjugate = keygen.genrotKey(sk.Get(), keygen.ckksContext.galElConjugate)
	}
}

// GenRotationKeysPow2 (:391).
func (keygen *keyGenerator) GenRotationKeysPow2(skOutput *SecretKey) (rotKey *RotationKeys) {
	if keygen.ckksContext.contextP == nil {
		panic("Cannot GenRotationKeysPow2: modulus P is empty")
	}
	rotKey = new(RotationKeys)
	rotKey.evakeyRotColLeft = make(map[uint64]*SwitchingKey)
	rotKey.evakeyRotColRight = make(map[uint64]*SwitchingKey)
	rotKey.permuteNTTLeftIndex = make(map[uint64][]uint64)
	rotKey.permuteNTTRightIndex = make(map[uint64][]uint64)
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
	for n := uint64(1); n < 1<<(keygen.params.LogN-1); n <<= 1 {
		rotKey.permuteNTTLeftIndex[n] = ring.PermuteNTTIndex(GaloisGen, n, keygen.ringContext.N)
		rotKey.permuteNTTRightIndex[n] = ring.PermuteNTTIndex(GaloisGen, 2*keygen.ringContext.N-n, keygen.ringContext.N)
		rotKey.evakeyRotColLeft[n] = add(keygen.ckksContext.galElRotColLeft[n])
		rotKey.evakeyRotColRight[n] = add(keygen.ckksContext.galElRotColRight[n])
	}
	rotKey.permuteNTTConjugateIndex = ring.PermuteNTTIndex(2*keygen.ringContext.N-1, 1, keygen.ringContext.N)
	rotKey.evakeyConjugate = add(keygen.ckksContext.galElConjugate)
	keygen.dev().GenRotationKeys(skOutput.Get(), galEls, noise, images)
	for i, k := range keys {
		keygen.finish(k, images[i])
	}
	return
}
