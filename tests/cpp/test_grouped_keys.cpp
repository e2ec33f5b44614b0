// The grouped aggregate verification over a resident key set through the C++ host mirror (include/bgls/bgls.hpp:
// KeySet::VerifyAggregateSignatureGroupedBySubset, KoskVerifyAggregateSignatureGroupedBySubset) against the older mirror functions on the
// gathered keys.  Built and run by tests/test_gpu_cpp_mirror_grouped_keys.py.
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

static void TestGroupedKeys(const CurveSystem* curve) {
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
  // nine signers, given in no order, over three messages (one of them empty)
  const std::vector<size_t> subset = {30, 2, 17, 5, 36, 0, 9, 21, 8};
  const std::vector<Bytes> texts = {randBytes(32), Bytes(), randBytes(5)};
  const size_t which[9] = {0, 1, 0, 2, 0, 1, 0, 0, 2};
  std::vector<Bytes> msgs;
  std::vector<Point> gathered, sigs, ksigs;
  for (size_t j = 0; j < 9; ++j) {
    msgs.push_back(texts[which[j]]);
    gathered.push_back(keys[subset[j]]);
    sigs.push_back(Sign(curve, sks[subset[j]], msgs[j]));
    ksigs.push_back(KoskSign(curve, sks[subset[j]], msgs[j]));
  }
  const Point agg = AggregateSignatures(sigs), kagg = AggregateSignatures(ksigs);
  size_t d = 99;
  CHECK(ks.VerifyAggregateSignatureGroupedBySubset(agg, subset, msgs, &d) && d == 3, "valid aggregate rejected");
  CHECK(VerifyAggregateSignatureGrouped(curve, agg, gathered, msgs), "the list form rejects the same aggregate on the gathered keys");
  CHECK(verifyAggSig(curve, agg, gathered, msgs, true), "the older path rejects the same aggregate on the gathered keys");
  CHECK(ks.KoskVerifyAggregateSignatureGroupedBySubset(kagg, subset, msgs, &d) && d == 3, "valid Kosk aggregate rejected");
  CHECK(!ks.KoskVerifyAggregateSignatureGroupedBySubset(agg, subset, msgs), "plain aggregate accepted by the Kosk form");
  std::vector<Bytes> bad = msgs;
  bad[4][31] ^= 1;                                        // that signer moves to a group of its own
  CHECK(!ks.VerifyAggregateSignatureGroupedBySubset(agg, subset, bad, &d) && d == 4, "tampered message accepted");
  std::vector<Bytes> moved = msgs;
  std::swap(moved[0], moved[1]);                          // two messages of different groups exchanged
  CHECK(!ks.VerifyAggregateSignatureGroupedBySubset(agg, subset, moved), "exchanged messages accepted");
  std::vector<size_t> other = subset;
  other[3] = 6;                                           // a non-signer in a signer's place: the same popcount
  CHECK(!ks.VerifyAggregateSignatureGroupedBySubset(agg, other, msgs), "another signer accepted");
  CHECK(!ks.VerifyAggregateSignatureGroupedBySubset(sigs[0], subset, msgs), "wrong signature accepted");
  CHECK(!ks.VerifyAggregateSignatureGroupedBySubset(foreign->GetG1(), subset, msgs), "foreign signature accepted");
  CHECK(!ks.VerifyAggregateSignatureGroupedBySubset(agg, subset, std::vector<Bytes>(msgs.begin(), msgs.begin() + 8)), "length mismatch accepted");
  CHECK(!ks.VerifyAggregateSignatureGroupedBySubset(agg, {2, 5, 2}, std::vector<Bytes>(msgs.begin(), msgs.begin() + 3)), "repeated index accepted");
  CHECK(!ks.VerifyAggregateSignatureGroupedBySubset(agg, {2, 5, N}, std::vector<Bytes>(msgs.begin(), msgs.begin() + 3)), "index outside the set accepted");
  CHECK(ks.VerifyAggregateSignatureGroupedBySubset(curve->GetG1Infinity(), {}, {}, &d) && d == 0, "no signer with sigma at infinity rejected");
  CHECK(!ks.VerifyAggregateSignatureGroupedBySubset(agg, {}, {}), "no signer with another sigma accepted");
  // everybody, three messages dealt round-robin
  std::vector<Bytes> every;
  std::vector<Point> esigs;
  for (size_t i = 0; i < N; ++i) {
    every.push_back(texts[i % 3]);
    esigs.push_back(Sign(curve, sks[i], every[i]));
  }
  const Point eagg = AggregateSignatures(esigs);
  CHECK(ks.VerifyAggregateSignatureGroupedBySubset(eagg, {}, every, &d, true) && d == 3, "everybody: valid aggregate rejected");
  CHECK(verifyAggSig(curve, eagg, keys, every, true), "everybody: the older path rejects the same aggregate");
  CHECK(!ks.VerifyAggregateSignatureGroupedBySubset(agg, {}, every, nullptr, true), "everybody: wrong signature accepted");
}

int main() {
  if (bgls_init(0) != 0) { std::printf("bgls_init failed: %s\n", bgls_last_error()); return 2; }
  for (const CurveSystem* curve : {Altbn128(), Bls12()}) TestGroupedKeys(curve);
  if (failures) { std::printf("%d FAILURES\n", failures); return 1; }
  std::printf("ALL OK\n");
  return 0;
}
