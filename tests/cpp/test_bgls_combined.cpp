// The combined multi-signature check through the C++ host mirror (include/bgls/bgls.hpp: VerifyMultiSignaturesCombined,
// KoskVerifyMultiSignaturesCombined, VerifyMultiSignaturesLocated) against the per-set mirror.  Built and run by
// tests/test_gpu_cpp_mirror_combined.py.
#include <cstdio>
#include <random>
#include "bgls/bgls.hpp"

using namespace curves;
using namespace bgls_go;

static std::mt19937_64 rng(20261018);
static Bytes randBytes(size_t n) { Bytes b(n); for (auto& x : b) x = (uint8_t)rng(); return b; }
static Bytes randScalar() { Bytes b = randBytes(32); b[0] &= 0x0f; return b; }   // < 2^252 < order
static int failures = 0;
#define CHECK(cond, what) do { if (!(cond)) { std::printf("FAIL %s: %s\n", curve->Name().c_str(), what); ++failures; } } while (0)

static void TestCombined(const CurveSystem* curve, bool kosk) {
  const size_t N = 9;
  std::vector<Bytes> msgs;
  std::vector<Point> sigs;
  std::vector<std::vector<Point>> keys;
  for (size_t b = 0; b < N; ++b) {
    msgs.push_back(randBytes(20 + b));
    std::vector<Point> ks, ss;
    for (size_t j = 0; j < 1 + b % 3; ++j) {
      Bytes sk = randScalar();
      ks.push_back(LoadPublicKey(curve, sk));
      ss.push_back(kosk ? KoskSign(curve, sk, msgs[b]) : Sign(curve, sk, msgs[b]));
    }
    keys.push_back(ks);
    sigs.push_back(AggregateSignatures(ss));
  }
  auto combined = [&](size_t group, bool* ok) {
    return kosk ? KoskVerifyMultiSignaturesCombined(curve, sigs, keys, msgs, group, Bytes(), ok) : VerifyMultiSignaturesCombined(curve, sigs, keys, msgs, group, Bytes(), ok);
  };
  bool ok = false;
  CHECK(combined(0, &ok) == std::vector<bool>({true}) && ok, "one valid group rejected");
  CHECK(combined(4, &ok) == std::vector<bool>({true, true, true}) && ok, "valid groups of four rejected");
  if (!kosk) CHECK(VerifyMultiSignaturesLocated(curve, sigs, keys, msgs, 4) == std::vector<bool>(N, true), "located: a valid set rejected");
  // the prefix matters
  std::vector<bool> other = kosk ? VerifyMultiSignaturesCombined(curve, sigs, keys, msgs, 0) : KoskVerifyMultiSignaturesCombined(curve, sigs, keys, msgs, 0);
  CHECK(other == std::vector<bool>({false}), "the other prefix accepted");
  sigs[5] = sigs[6];
  CHECK(combined(0, &ok) == std::vector<bool>({false}) && ok, "a bad set inside one group accepted");
  CHECK(combined(4, &ok) == std::vector<bool>({true, false, true}) && ok, "the bad set's group not isolated");
  if (!kosk) {
    std::vector<bool> want = verifyMultiSignatures(curve, sigs, keys, msgs);
    CHECK(want[5] == false && VerifyMultiSignaturesLocated(curve, sigs, keys, msgs, 4) == want, "located differs from the per-set verdicts");
    CHECK(VerifyMultiSignaturesLocated(curve, sigs, keys, msgs, 0) == want, "located with one group differs from the per-set verdicts");
  }
  // a seed of the wrong length and a foreign point: the call does not run
  CHECK(VerifyMultiSignaturesCombined(curve, sigs, keys, msgs, 0, Bytes(5, 1), &ok) == std::vector<bool>({false}) && !ok, "short seed accepted");
  const CurveSystem* foreign = curve == Altbn128() ? Bls12() : Altbn128();
  std::vector<Point> s2 = sigs;
  s2[0] = foreign->GetG1();
  CHECK(VerifyMultiSignaturesCombined(curve, s2, keys, msgs, 0, Bytes(), &ok) == std::vector<bool>({false}) && !ok, "foreign signature accepted");
}

int main() {
  if (bgls_init(0) != 0) { std::printf("bgls_init failed: %s\n", bgls_last_error()); return 2; }
  for (const CurveSystem* curve : {Altbn128(), Bls12()}) { TestCombined(curve, false); TestCombined(curve, true); }
  if (failures) { std::printf("%d FAILURES\n", failures); return 1; }
  std::printf("ALL OK\n");
  return 0;
}
