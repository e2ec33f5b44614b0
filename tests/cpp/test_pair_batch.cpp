// CurveSystem::PairBatch through the C++ host mirror (include/bgls/curves.hpp) against a list of Pair results, with the C calls
// bgls_pair_batch and bgls_final_exp_batch beside it.  Built and run by tests/test_gpu_cpp_mirror_pair_batch.py.
#include <cstdio>
#include <random>
#include "bgls/curves.hpp"

using namespace curves;

static std::mt19937_64 rng(20261020);
static Bytes randScalar() { Bytes b(32); for (auto& x : b) x = (uint8_t)rng(); b[0] &= 0x0f; return b; }   // < 2^252 < order
static int failures = 0;
#define CHECK(cond, what) do { if (!(cond)) { std::printf("FAIL %s: %s\n", curve->Name().c_str(), what); ++failures; } } while (0)

static void TestPairBatch(const CurveSystem* curve) {
  const size_t N = 13;                                    // more than the ten items of one wave
  std::vector<Point> p1, p2;
  for (size_t b = 0; b < N; ++b) {
    p1.push_back(curve->GetG1().Mul(randScalar()));
    p2.push_back(curve->GetG2().Mul(randScalar(), b % 2 == 1));
  }
  p1[3] = curve->GetG1Infinity();
  p2[7] = curve->GetG2Infinity();
  p1[9] = curve->GetG1();
  p2[9] = curve->GetG2();
  std::vector<PointT> got = curve->PairBatch(p1, p2);
  CHECK(got.size() == N, "wrong length");
  for (size_t b = 0; b < N && b < got.size(); ++b) {
    auto want = curve->Pair(p1[b], p2[b]);
    CHECK(want.second && got[b].valid() && got[b].Equals(want.first), "an item differs from Pair");
  }
  if (got.size() == N) {
    CHECK(got[3].Equals(curve->GetGTIdentity()) && got[7].Equals(curve->GetGTIdentity()), "a pair with infinity is not one");
    CHECK(!got[9].Equals(curve->GetGTIdentity()), "e(g1, g2) is one");
  }
  CHECK(curve->PairBatch(p1, std::vector<Point>(p2.begin(), p2.end() - 1)).empty(), "lengths that differ gave a list");
  CHECK(curve->PairBatch({}, {}).empty(), "an empty call gave items");
  // a foreign point: that item is Pair's (nil, false), the others are still the batch's
  const CurveSystem* foreign = curve == Altbn128() ? Bls12() : Altbn128();
  std::vector<Point> q1 = p1;
  q1[5] = foreign->GetG1();
  std::vector<PointT> mixed = curve->PairBatch(q1, p2);
  CHECK(mixed.size() == N && !mixed[5].valid(), "a foreign point gave a value");
  for (size_t b = 0; b < N && b < mixed.size(); ++b)
    if (b != 5) CHECK(mixed[b].Equals(got[b]), "an item beside a foreign point differs");
  // an off-curve point fails the C call as a whole; the mirror settles item by item
  std::vector<Point> r1 = p1;
  r1[6].raw.back() ^= 1;
  Bytes g1, g2, o(N * bgls_gt_size(curve->id), 0x5a);
  for (size_t b = 0; b < N; ++b) {
    g1.insert(g1.end(), r1[b].raw.begin(), r1[b].raw.end());
    g2.insert(g2.end(), p2[b].raw.begin(), p2[b].raw.end());
  }
  CHECK(bgls_pair_batch(curve->id, g1.data(), g2.data(), N, o.data()) == BGLS_ERR_ENCODING, "an off-curve point did not fail the call");
  CHECK(o == Bytes(o.size(), 0x5a), "a failed call wrote its output");
  std::vector<PointT> settled = curve->PairBatch(r1, p2);
  CHECK(settled.size() == N && !settled[6].valid(), "an off-curve point gave a value");
  for (size_t b = 0; b < N && b < settled.size(); ++b)
    if (b != 6) CHECK(settled[b].Equals(got[b]), "an item beside an off-curve point differs");
  // bgls_final_exp_batch over the pairing values: is_one marks exactly the items whose bytes are one, and one stays one
  Bytes in, out(N * bgls_gt_size(curve->id)), one(N, 7);
  for (size_t b = 0; b < N; ++b) in.insert(in.end(), got[b].raw.begin(), got[b].raw.end());
  CHECK(bgls_final_exp_batch(curve->id, in.data(), N, out.data(), one.data()) == 0, "bgls_final_exp_batch failed");
  for (size_t b = 0; b < N; ++b) {
    const Bytes item(out.begin() + b * bgls_gt_size(curve->id), out.begin() + (b + 1) * bgls_gt_size(curve->id));
    CHECK(one[b] == (item == curve->GetGTIdentity().raw ? 1 : 0), "is_one disagrees with the bytes");
    if (b == 3 || b == 7) CHECK(one[b] == 1, "the final exponentiation of one is not one");
  }
}

int main() {
  if (bgls_init(0) != 0) { std::printf("bgls_init failed: %s\n", bgls_last_error()); return 2; }
  for (const CurveSystem* curve : {Altbn128(), Bls12()}) TestPairBatch(curve);
  if (failures) { std::printf("%d FAILURES\n", failures); return 1; }
  std::printf("ALL OK\n");
  return 0;
}
