// Recording stand-ins for the launchers of lr_bfv_encrypt.hip (stub_touch.hpp says what a stand-in does): each records its name with the
// count of shared-stub launches before it, from which a driver reads the call order.
#include <atomic>
#include <mutex>
#include <string>
#include <vector>

#include "lr_device.hpp"
#include "stub_touch.hpp"

namespace lr {

extern std::atomic<unsigned long long> g_stub_launches;
std::atomic<unsigned long long> g_encryptor_stub_launches{0};
struct EncryptorStubEvent {
    std::string name;
    unsigned long long shared_before;     // g_stub_launches when the launch was made
    int limbs, batch;
};
thread_local std::vector<EncryptorStubEvent> t_encryptor_stub_events;     // per thread: two handles on two threads record apart

namespace {
void record(const char *name, int limbs, int batch) {
    g_encryptor_stub_launches.fetch_add(1);
    t_encryptor_stub_events.push_back(EncryptorStubEvent{name, g_stub_launches.load(), limbs, batch});
}
}  // namespace

// the calling thread's record, for the driver
void encryptor_stub_clear() { t_encryptor_stub_events.clear(); }
int encryptor_stub_count() { return (int)t_encryptor_stub_events.size(); }
const char *encryptor_stub_name(int i) { return t_encryptor_stub_events[(size_t)i].name.c_str(); }
unsigned long long encryptor_stub_shared_before(int i) { return t_encryptor_stub_events[(size_t)i].shared_before; }
int encryptor_stub_limbs(int i) { return t_encryptor_stub_events[(size_t)i].limbs; }
int encryptor_stub_batch(int i) { return t_encryptor_stub_events[(size_t)i].batch; }

hipError_t launch_bfv_ternary(const TernaryLaunch &L, int limbs, int batch, hipStream_t) {
    if (const LaunchVerdict v = launch_verdict(L, limbs, batch)) return verdict_error(v);
    record("ternary", limbs, batch);
    for (int b = 0; b < batch; ++b) {
        rd(L.coeff_bits + (long long)b * (L.n >> 3), L.n >> 3);
        rd(L.sign_bits + (long long)b * (L.n >> 3), L.n >> 3);
        for (int i = 0; i < limbs; ++i) wr(L.out + b * L.out_stride + (long long)i * L.n, L.n);
    }
    return hipSuccess;
}

hipError_t launch_bfv_noise(const NoiseLaunch &L, int comps, int limbs, int batch, hipStream_t) {
    if (const LaunchVerdict v = launch_verdict(L, comps, limbs, batch)) return verdict_error(v);
    record(L.add ? (comps == 2 ? "noise_add2" : "noise_add") : "noise_expand", limbs, batch);
    rd(L.lp, limbs);
    for (int k = 0; k < comps; ++k)
        for (int b = 0; b < batch; ++b) {
            rd(L.e[k] + (long long)b * L.n, L.n);
            for (int i = 0; i < limbs; ++i) {
                if (L.add) rd(L.x[k] + b * L.x_stride[k] + (long long)i * L.n, L.n);
                if (L.add && L.plus[k]) rd(L.plus[k] + b * L.plus_stride[k] + (long long)i * L.n, L.n);
                wr(L.out[k] + b * L.out_stride[k] + (long long)i * L.n, L.n);
            }
        }
    return hipSuccess;
}

hipError_t launch_bfv_negmul(const NegMulLaunch &L, int limbs, int batch, hipStream_t) {
    if (const LaunchVerdict v = launch_verdict(L, limbs, batch)) return verdict_error(v);
    record("negmul", limbs, batch);
    rd(L.lp, limbs);
    for (int b = 0; b < batch; ++b)
        for (int i = 0; i < limbs; ++i) {
            rd(L.a + b * L.a_stride + (long long)i * L.n, L.n);
            rd(L.b + b * L.b_stride + (long long)i * L.n, L.n);
            wr(L.out + b * L.out_stride + (long long)i * L.n, L.n);
        }
    return hipSuccess;
}

}  // namespace lr
