// Multi-signatures by signer subset of a resident key set through the C++ host mirror (include/bgls/bgls.hpp: KeySet::AggregateKeysBySubset,
// KeySet::VerifyMultiSignaturesBySubset, KeySet::KoskVerifyMultiSignaturesBySubset) against AggregateKeys / verifyMultiSignature /
// KoskVerifyMultiSignature on the gathered keys.  Built and run by tests/test_gpu_cpp_mirror_subsets.py.
#include <cstdio>
#include <random>
#include "bgls/bgls.hpp"

using namespace curves;
using namespace bgls_go;

static std::mt19937_64 rng(20261020);
static Bytes randBytes(size_t n) { Bytes b(n); for (auto& x : b) x = (uint8_t)rng(); return b; }
static Bytes randScalar() { Bytes b = randBytes(32); b[0] &= 0x0f; return b; }   // < 2^252 < order
static int failures = 0;
#define CHECK(cond, what) do { if (!(cond)) { std::printf("FAIL %s: %s\n", curve->Name().c_str(), what); ++failures; } } while (0)

static void TestSubsets(const CurveSystem* curve) {
  const size_t N = 37;
  const CurveSystem* foreign = curve == Altbn128() ? Bls12() : Altbn128();
  std::vector<Bytes> sks;
  std::vector<Point> keys;
  for (size_t i = 0; i < N; ++i) {
    sks.push_back(randScalar());
    keys.push_back(LoadPublicKey(curve, sks[i]));
  }
  KeySet ks(curve, keys);
  CHECK(ks.ok() && ks.size() == N, "upload failed");
  std::vector<size_t> all, most, few = {0, 7, 36};
  for (size_t i = 0; i < N; ++i) {
    all.push_back(i);
    if (i != 5) most.push_back(i);
  }
  const std::vector<std::vector<size_t>> subsets = {few, all, most, {36}, {3, 3, 4}};
  std::vector<Bytes> msgs;
  std::vector<Point> sigs, ksigs;
  std::vector<std::vector<Point>> gathered;
  for (size_t b = 0; b < subsets.size(); ++b) {
    msgs.push_back(randBytes(5 + 3 * b));
    std::vector<bool> in(N, false);
    for (size_t i : subsets[b]) in[i] = true;
    std::vector<Point> ss, kss, kk;
    for (size_t i = 0; i < N; ++i)
      if (in[i]) {
        ss.push_back(Sign(curve, sks[i], msgs[b]));
        kss.push_back(KoskSign(curve, sks[i], msgs[b]));
        kk.push_back(keys[i]);
      }
    sigs.push_back(AggregateSignatures(ss));
    ksigs.push_back(AggregateSignatures(kss));
    gathered.push_back(kk);
  }
  const std::vector<Point> sums = ks.AggregateKeysBySubset(subsets);
  CHECK(sums.size() == subsets.size(), "AggregateKeysBySubset failed");
  for (size_t b = 0; b < sums.size(); ++b) CHECK(sums[b].Equals(AggregateKeys(gathered[b])), "a subset's key sum differs from AggregateKeys of the gathered keys");
  CHECK(ks.AggregateKeysBySubset({{N}}).empty(), "an index outside the set was accepted");
  // one wrong signature, one foreign point, one changed message
  std::vector<Point> s2 = sigs, k2 = ksigs;
  std::vector<Bytes> m2 = msgs;
  s2[1] = sigs[0];
  k2[1] = ksigs[0];
  s2[3] = foreign->GetG1();
  k2[3] = foreign->GetG1();
  m2[4][0] ^= 1;
  std::vector<bool> want, kwant;
  for (size_t b = 0; b < subsets.size(); ++b) {
    want.push_back(verifyMultiSignature(curve, s2[b], gathered[b], m2[b]));
    kwant.push_back(KoskVerifyMultiSignature(curve, k2[b], gathered[b], m2[b]));
  }
  CHECK(want == std::vector<bool>({true, false, true, false, false}), "single verdicts");
  CHECK(kwant == want, "single Kosk verdicts");
  CHECK(ks.VerifyMultiSignaturesBySubset(s2, subsets, m2) == want, "subset batch differs from the single calls");
  CHECK(ks.KoskVerifyMultiSignaturesBySubset(k2, subsets, m2) == kwant, "Kosk subset batch differs from the single calls");
  CHECK(ks.VerifyMultiSignaturesBySubset(sigs, subsets, msgs) == std::vector<bool>(subsets.size(), true), "valid sets rejected");
}

int main() {
  if (bgls_init(0) != 0) { std::printf("bgls_init failed: %s\n", bgls_last_error()); return 2; }
  for (const CurveSystem* curve : {Altbn128(), Bls12()}) TestSubsets(curve);
  if (failures) { std::printf("%d FAILURES\n", failures); return 1; }
  std::printf("ALL OK\n");
  return 0;
}
