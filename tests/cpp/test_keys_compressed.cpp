// Key sets from compressed keys through the C++ host mirror (include/bgls/bgls.hpp: KeySet::FromCompressed, KeySet::Read) against a set
// uploaded from the same keys uncompressed.  Built and run by tests/test_gpu_keys_compressed.py.
#include <cstdio>
#include <random>
#include "bgls/bgls.hpp"

using namespace curves;
using namespace bgls_go;

static std::mt19937_64 rng(20261021);
static Bytes randBytes(size_t n) { Bytes b(n); for (auto& x : b) x = (uint8_t)rng(); return b; }
static Bytes randScalar() { Bytes b = randBytes(32); b[0] &= 0x0f; return b; }   // < 2^252 < order
static int failures = 0;
#define CHECK(cond, what) do { if (!(cond)) { std::printf("FAIL %s: %s\n", curve->Name().c_str(), what); ++failures; } } while (0)

static void TestCompressed(const CurveSystem* curve) {
  const size_t N = 9;
  std::vector<Bytes> sks, msgs;
  std::vector<Point> keys, sigs;
  Bytes comp;
  for (size_t i = 0; i < N; ++i) {
    sks.push_back(randScalar());
    keys.push_back(LoadPublicKey(curve, sks[i]));
    msgs.push_back(randBytes(4 + i));
    sigs.push_back(Sign(curve, sks[i], msgs[i]));
    const Bytes c = keys[i].Marshal();
    comp.insert(comp.end(), c.begin(), c.end());
  }
  size_t bad = 12345;
  auto ks = KeySet::FromCompressed(curve, comp, {}, false, &bad);
  CHECK(ks->ok() && ks->size() == N && bad == 12345, "upload of compressed keys failed");
  const std::vector<Point> back = ks->Read();
  CHECK(back.size() == N, "Read failed");
  for (size_t i = 0; i < back.size(); ++i) CHECK(back[i].Equals(keys[i]), "a key read back differs from the key that was compressed");
  const Point agg = AggregateSignatures(sigs);
  CHECK(ks->VerifyAggregateSignature(agg, msgs), "valid aggregate rejected on the set from compressed keys");
  msgs[3][0] ^= 1;
  CHECK(!ks->VerifyAggregateSignature(agg, msgs), "changed message accepted");
  // key 4 broken: x -> x + 1 is on the twist with probability 1/2 and in the subgroup with probability ~0
  Bytes broken = comp;
  const size_t cb = comp.size() / N;
  broken[4 * cb + cb - 1] ^= 1;
  auto none = KeySet::FromCompressed(curve, broken, {}, false, &bad);
  CHECK(!none->ok() && bad == 4, "a refused key was not reported at its index");
  CHECK(none->Read().empty(), "a failed set can be read");
  CHECK(!KeySet::FromCompressed(curve, Bytes(cb + 1))->ok(), "a ragged length was accepted");
}

int main() {
  if (bgls_init(0) != 0) { std::printf("bgls_init failed: %s\n", bgls_last_error()); return 2; }
  for (const CurveSystem* curve : {Altbn128(), Bls12()}) TestCompressed(curve);
  if (failures) { std::printf("%d FAILURES\n", failures); return 1; }
  std::printf("ALL OK\n");
  return 0;
}
