// The aggregate verification that pairs once per distinct message through the C++ host mirror (include/bgls/bgls.hpp: GroupMessages,
// VerifyAggregateSignatureGrouped, KoskVerifyAggregateSignatureGrouped) against the older mirror functions on the same inputs.  Built and
// run by tests/test_gpu_cpp_mirror_grouped.py.
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

static void TestGrouped(const CurveSystem* curve) {
  const CurveSystem* foreign = curve == Altbn128() ? Bls12() : Altbn128();
  // nine signers over three messages (one of them empty), in a mixed order
  const std::vector<Bytes> texts = {randBytes(32), Bytes(), randBytes(5)};
  const size_t which[9] = {0, 1, 0, 2, 0, 1, 0, 0, 2};
  std::vector<Bytes> sks, msgs;
  std::vector<Point> keys, sigs, ksigs;
  for (size_t i = 0; i < 9; ++i) {
    sks.push_back(randScalar());
    msgs.push_back(texts[which[i]]);
    keys.push_back(LoadPublicKey(curve, sks[i]));
    sigs.push_back(Sign(curve, sks[i], msgs[i]));
    ksigs.push_back(KoskSign(curve, sks[i], msgs[i]));
  }
  std::vector<uint32_t> group_of;
  size_t d = 99;
  CHECK(GroupMessages(msgs, group_of, d), "GroupMessages failed");
  CHECK(d == 3 && group_of == std::vector<uint32_t>({0, 1, 0, 2, 0, 1, 0, 0, 2}), "groups are not numbered by first occurrence");
  const Point agg = AggregateSignatures(sigs), kagg = AggregateSignatures(ksigs);
  d = 99;
  CHECK(VerifyAggregateSignatureGrouped(curve, agg, keys, msgs, &d) && d == 3, "valid aggregate rejected");
  CHECK(verifyAggSig(curve, agg, keys, msgs, true), "the older path rejects the same aggregate");
  CHECK(KoskVerifyAggregateSignatureGrouped(curve, kagg, keys, msgs, &d) && d == 3, "valid Kosk aggregate rejected");
  CHECK(KoskVerifyAggregateSignature(curve, kagg, keys, msgs), "the older Kosk path rejects the same aggregate");
  CHECK(!KoskVerifyAggregateSignatureGrouped(curve, agg, keys, msgs), "plain aggregate accepted by the Kosk form");
  std::vector<Bytes> bad = msgs;
  bad[4][31] ^= 1;                                        // signer 4 moves to a group of its own
  CHECK(!VerifyAggregateSignatureGrouped(curve, agg, keys, bad, &d) && d == 4, "tampered message accepted");
  CHECK(!verifyAggSig(curve, agg, keys, bad, true), "the older path accepts the tampered message");
  std::vector<Bytes> moved = msgs;
  std::swap(moved[0], moved[1]);                          // two messages of different groups exchanged
  CHECK(!VerifyAggregateSignatureGrouped(curve, agg, keys, moved), "exchanged messages accepted");
  std::vector<Point> swapped = keys;
  std::swap(swapped[0], swapped[2]);                      // two signers of ONE message exchanged: the same key sums
  CHECK(VerifyAggregateSignatureGrouped(curve, agg, swapped, msgs), "exchange within a group rejected");
  CHECK(!VerifyAggregateSignatureGrouped(curve, sigs[0], keys, msgs), "wrong signature accepted");
  CHECK(!VerifyAggregateSignatureGrouped(curve, foreign->GetG1(), keys, msgs), "foreign signature accepted");
  CHECK(!VerifyAggregateSignatureGrouped(curve, agg, keys, std::vector<Bytes>(msgs.begin(), msgs.begin() + 8)), "length mismatch accepted");
  CHECK(VerifyAggregateSignatureGrouped(curve, curve->GetG1Infinity(), {}, {}, &d) && d == 0, "the empty instance with sigma at infinity rejected");
  CHECK(!VerifyAggregateSignatureGrouped(curve, agg, {}, {}), "the empty instance with another sigma accepted");
}

int main() {
  if (bgls_init(0) != 0) { std::printf("bgls_init failed: %s\n", bgls_last_error()); return 2; }
  for (const CurveSystem* curve : {Altbn128(), Bls12()}) TestGrouped(curve);
  if (failures) { std::printf("%d FAILURES\n", failures); return 1; }
  std::printf("ALL OK\n");
  return 0;
}
