// The distinct-message and key-possession checks through the C++ host mirror (include/bgls/bgls.hpp: DistinctMsgVerifyAggregateSignature(s),
// DistinctMsgVerifySingleSignature(s), CheckAuthentication(s), KeySet::DistinctMsgVerifyAggregateSignature, CurveSystem::HashToG1Keyed)
// against the older mirror functions fed messages prefixed here.  Built and run by tests/test_gpu_cpp_mirror_distinct.py.
#include <cstdio>
#include <random>
#include "bgls/bgls.hpp"

using namespace curves;
using namespace bgls_go;

static std::mt19937_64 rng(20261019);
static Bytes randBytes(size_t n) { Bytes b(n); for (auto& x : b) x = (uint8_t)rng(); return b; }
static Bytes randScalar() { Bytes b = randBytes(32); b[0] &= 0x0f; return b; }   // < 2^252 < order
static int failures = 0;
#define CHECK(cond, what) do { if (!(cond)) { std::printf("FAIL %s: %s\n", curve->Name().c_str(), what); ++failures; } } while (0)

static Bytes prefixed(const Point& key, const Bytes& msg) {
  Bytes m = key.MarshalUncompressed();
  m.insert(m.end(), msg.begin(), msg.end());
  return m;
}

static void TestDistinct(const CurveSystem* curve) {
  const size_t N = 7;
  const CurveSystem* foreign = curve == Altbn128() ? Bls12() : Altbn128();
  std::vector<Bytes> sks, msgs, pre;
  std::vector<Point> keys, sigs, auths;
  for (size_t i = 0; i < N; ++i) {
    sks.push_back(randScalar());
    msgs.push_back(randBytes(3 * i));
    keys.push_back(LoadPublicKey(curve, sks[i]));
    pre.push_back(prefixed(keys[i], msgs[i]));
    sigs.push_back(DistinctMsgSign(curve, sks[i], msgs[i]));
    auths.push_back(Authenticate(curve, sks[i]));
    CHECK(sigs[i].Equals(Sign(curve, sks[i], pre[i])), "DistinctMsgSign differs from Sign on the prefixed message");
    CHECK(auths[i].Equals(Sign(curve, sks[i], keys[i].Marshal())), "Authenticate differs from Sign on the compressed key");
  }
  std::vector<Point> hk = curve->HashToG1Keyed(keys, &msgs), hp = curve->HashToG1Keyed(keys);
  CHECK(hk.size() == N && hp.size() == N, "HashToG1Keyed failed");
  for (size_t i = 0; i < N && hk.size() == N && hp.size() == N; ++i) {
    CHECK(hk[i].Equals(curve->HashToG1(pre[i])), "HashToG1Keyed differs from HashToG1 of key || message");
    CHECK(hp[i].Equals(curve->HashToG1(keys[i].Marshal())), "HashToG1Keyed differs from HashToG1 of the compressed key");
  }
  const Point agg = AggregateSignatures(sigs);
  CHECK(DistinctMsgVerifyAggregateSignature(curve, agg, keys, msgs), "valid aggregate rejected");
  CHECK(verifyAggSig(curve, agg, keys, pre, true), "the older path rejects the same aggregate");
  std::vector<Bytes> bad = msgs;
  bad[3][0] ^= 1;
  CHECK(!DistinctMsgVerifyAggregateSignature(curve, agg, keys, bad), "tampered message accepted");
  std::vector<Point> swapped = keys;
  std::swap(swapped[0], swapped[1]);
  CHECK(!DistinctMsgVerifyAggregateSignature(curve, agg, swapped, msgs), "exchanged keys accepted");
  KeySet ks(curve, keys);
  CHECK(ks.ok() && ks.DistinctMsgVerifyAggregateSignature(agg, msgs), "key set: valid aggregate rejected");
  CHECK(!ks.DistinctMsgVerifyAggregateSignature(agg, bad), "key set: tampered message accepted");
  // batches against the lists of single calls, with a foreign point and a length mismatch among the items
  std::vector<Point> s3(sigs.begin(), sigs.begin() + 3), k3(keys.begin(), keys.begin() + 3);
  std::vector<Bytes> m3(msgs.begin(), msgs.begin() + 3), m2(msgs.begin(), msgs.begin() + 2);
  const Point agg3 = AggregateSignatures(s3);
  std::vector<Point> isigs = {agg, agg3, agg3, foreign->GetG1(), agg3};
  std::vector<std::vector<Point>> ikeys = {keys, k3, k3, k3, k3};
  std::vector<std::vector<Bytes>> imsgs = {msgs, m3, std::vector<Bytes>(bad.begin() + 1, bad.begin() + 4), m3, m2};
  std::vector<bool> want;
  for (size_t b = 0; b < isigs.size(); ++b) want.push_back(DistinctMsgVerifyAggregateSignature(curve, isigs[b], ikeys[b], imsgs[b]));
  CHECK(want == std::vector<bool>({true, true, false, false, false}), "single aggregate verdicts");
  CHECK(DistinctMsgVerifyAggregateSignatures(curve, isigs, ikeys, imsgs) == want, "aggregate batch differs from the single calls");
  std::vector<Point> osigs = sigs, okeys = keys, oauths = auths;
  osigs[2] = sigs[1];
  okeys[4] = keys[5];
  osigs[6] = foreign->GetG1();
  oauths[2] = auths[1];
  oauths[6] = foreign->GetG1();
  std::vector<bool> w1, w2;
  for (size_t i = 0; i < N; ++i) {
    w1.push_back(DistinctMsgVerifySingleSignature(curve, osigs[i], okeys[i], msgs[i]));
    w2.push_back(CheckAuthentication(curve, okeys[i], oauths[i]));
    if (osigs[i].curve == curve) CHECK(w1[i] == VerifySingleSignature(curve, osigs[i], okeys[i], prefixed(okeys[i], msgs[i])), "single differs from the older path");
    if (oauths[i].curve == curve) CHECK(w2[i] == VerifySingleSignature(curve, oauths[i], okeys[i], okeys[i].Marshal()), "authentication differs from the older path");
  }
  CHECK(w1 == std::vector<bool>({true, true, false, true, false, true, false}), "single verdicts");
  CHECK(w2 == w1, "authentication verdicts");
  CHECK(DistinctMsgVerifySingleSignatures(curve, osigs, okeys, msgs) == w1, "single batch differs from the single calls");
  CHECK(CheckAuthentications(curve, okeys, oauths) == w2, "authentication batch differs from the single calls");
}

int main() {
  if (bgls_init(0) != 0) { std::printf("bgls_init failed: %s\n", bgls_last_error()); return 2; }
  for (const CurveSystem* curve : {Altbn128(), Bls12()}) TestDistinct(curve);
  if (failures) { std::printf("%d FAILURES\n", failures); return 1; }
  std::printf("ALL OK\n");
  return 0;
}
