// C++ host-side mirror of the reference's Go package `bgls` on the hot path (bgls/bgls.go,
// bgls/blsKosk.go): same function names and semantics, each verification = ONE batch C call.
#pragma once
#include <random>
#include "curves.hpp"

namespace bgls_go {   // "package bgls"; the name bgls:: is taken by the kernels' namespace

using curves::Bytes;
using curves::CurveSystem;
using curves::Point;

// bgls/bgls.go:40-43
inline Point LoadPublicKey(const CurveSystem* curve, const Bytes& sk_be32) { return curve->GetG2().Mul(sk_be32); }
// bgls/bgls.go:46-56
inline Point Sign(const CurveSystem* curve, const Bytes& sk_be32, const Bytes& msg) { return curve->HashToG1(msg).Mul(sk_be32); }
// bgls/blsKosk.go:73-77
inline Point KoskSign(const CurveSystem* curve, const Bytes& sk_be32, const Bytes& msg) {
  Bytes m(1, 1);
  m.insert(m.end(), msg.begin(), msg.end());
  return Sign(curve, sk_be32, m);
}
// bgls/bgls.go:123-131
inline Point AggregateSignatures(const std::vector<Point>& sigs) { return curves::AggregatePoints(sigs); }
inline Point AggregateKeys(const std::vector<Point>& keys) { return curves::AggregatePoints(keys); }

// verifyAggSig, bgls/bgls.go:94-119
inline bool verifyAggSig(const CurveSystem* curve, const Point& aggsig, const std::vector<Point>& keys,
                         const std::vector<Bytes>& msgs, bool allowDuplicates) {
  if (keys.size() != msgs.size()) return false;
  if (aggsig.curve != curve || aggsig.group != BGLS_G1) return false;
  Bytes kb, blob;
  std::vector<uint64_t> off(msgs.size() + 1, 0);
  for (size_t i = 0; i < keys.size(); ++i) {
    if (keys[i].curve != curve || keys[i].group != BGLS_G2) return false;
    kb.insert(kb.end(), keys[i].raw.begin(), keys[i].raw.end());
    off[i] = blob.size();
    blob.insert(blob.end(), msgs[i].begin(), msgs[i].end());
  }
  off[msgs.size()] = blob.size();
  return bgls_verify_aggregate(curve->id, aggsig.raw.data(), kb.data(), blob.data(), off.data(), keys.size(), allowDuplicates ? 1 : 0) == 1;
}
// bgls/bgls.go:82-84
inline bool VerifyAggregateSignature(const CurveSystem* curve, const Point& aggsig, const std::vector<Point>& keys,
                                     const std::vector<Bytes>& msgs) {
  return verifyAggSig(curve, aggsig, keys, msgs, false);
}
// bgls/blsKosk.go:100-106
inline bool KoskVerifyAggregateSignature(const CurveSystem* curve, const Point& aggsig, const std::vector<Point>& keys,
                                         const std::vector<Bytes>& msgs) {
  std::vector<Bytes> m2;
  for (const Bytes& m : msgs) {
    Bytes x(1, 1);
    x.insert(x.end(), m.begin(), m.end());
    m2.push_back(x);
  }
  return verifyAggSig(curve, aggsig, keys, m2, true);
}

// group_of[i] = the number of the group of msgs[i]: two messages share a group iff their bytes are equal, groups are numbered in the order
// of their first occurrence (bgls_group_messages: the grouping runs on the device).  false: the call failed, see bgls_last_error().
inline bool GroupMessages(const std::vector<Bytes>& msgs, std::vector<uint32_t>& group_of, size_t& n_groups) {
  Bytes blob;
  std::vector<uint64_t> off(msgs.size() + 1, 0);
  for (size_t i = 0; i < msgs.size(); ++i) {
    off[i] = blob.size();
    blob.insert(blob.end(), msgs[i].begin(), msgs[i].end());
  }
  off[msgs.size()] = blob.size();
  group_of.assign(msgs.size(), 0);
  n_groups = 0;
  return bgls_group_messages(blob.data(), off.data(), msgs.size(), group_of.data(), &n_groups) == 0;
}
// verifyAggSig with allowDuplicates = true (KoskVerifyAggregateSignature's body, bgls/blsKosk.go:100-106) with one hash and one pairing per
// DISTINCT message: the keys of the signers of one message are summed first (bgls_verify_aggregate_grouped).  Same verdict; messages are
// grouped by exact bytes; no duplicate rule.  For keys resident in a KeySet use its signer-bitmap calls (VerifyMultiSignaturesBySubset).
inline bool VerifyAggregateSignatureGrouped(const CurveSystem* curve, const Point& aggsig, const std::vector<Point>& keys,
                                            const std::vector<Bytes>& msgs, size_t* n_groups = nullptr) {
  if (keys.size() != msgs.size()) return false;
  if (aggsig.curve != curve || aggsig.group != BGLS_G1) return false;
  Bytes kb, blob;
  std::vector<uint64_t> off(msgs.size() + 1, 0);
  for (size_t i = 0; i < keys.size(); ++i) {
    if (keys[i].curve != curve || keys[i].group != BGLS_G2) return false;
    kb.insert(kb.end(), keys[i].raw.begin(), keys[i].raw.end());
    off[i] = blob.size();
    blob.insert(blob.end(), msgs[i].begin(), msgs[i].end());
  }
  off[msgs.size()] = blob.size();
  return bgls_verify_aggregate_grouped(curve->id, aggsig.raw.data(), kb.data(), blob.data(), off.data(), keys.size(), n_groups, nullptr) == 1;
}
// bgls/blsKosk.go:100-106, grouped
inline bool KoskVerifyAggregateSignatureGrouped(const CurveSystem* curve, const Point& aggsig, const std::vector<Point>& keys,
                                                const std::vector<Bytes>& msgs, size_t* n_groups = nullptr) {
  std::vector<Bytes> m2;
  for (const Bytes& m : msgs) {
    Bytes x(1, 1);
    x.insert(x.end(), m.begin(), m.end());
    m2.push_back(x);
  }
  return VerifyAggregateSignatureGrouped(curve, aggsig, keys, m2, n_groups);
}
// verifyMultiSignature, bgls/bgls.go:89-92
inline bool verifyMultiSignature(const CurveSystem* curve, const Point& aggsig, const std::vector<Point>& keys, const Bytes& msg) {
  if (aggsig.curve != curve || aggsig.group != BGLS_G1) return false;      // a nil / foreign aggsig is `false`
  Bytes kb;
  for (const Point& k : keys) {
    if (k.curve != curve || k.group != BGLS_G2) return false;
    kb.insert(kb.end(), k.raw.begin(), k.raw.end());
  }
  return bgls_verify_multi(curve->id, aggsig.raw.data(), kb.data(), keys.size(), msg.data(), msg.size()) == 1;
}
// bgls/bgls.go:59-70
inline bool VerifySingleSignature(const CurveSystem* curve, const Point& sig, const Point& pubKey, const Bytes& msg) {
  return verifyMultiSignature(curve, sig, {pubKey}, msg);
}
// bgls/blsKosk.go:117-120
inline bool KoskVerifyMultiSignature(const CurveSystem* curve, const Point& aggsig, const std::vector<Point>& keys, const Bytes& msg) {
  Bytes m(1, 1);
  m.insert(m.end(), msg.begin(), msg.end());
  return verifyMultiSignature(curve, aggsig, keys, m);
}

// A []Point of public keys resident on the GPU(s) (bgls_keys_t): uploaded, parsed and validated once, verified many times.
class KeySet {
 public:
  KeySet(const CurveSystem* curve, const std::vector<Point>& keys, const std::vector<int>& devices = {}, bool check = true) : curve_(curve), n_(keys.size()) {
    Bytes kb;
    for (const Point& k : keys) {
      if (k.curve != curve || k.group != BGLS_G2) return;
      kb.insert(kb.end(), k.raw.begin(), k.raw.end());
    }
    const int nd = devices.empty() ? 1 : (int)devices.size();
    ok_ = bgls_keys_upload(curve->id, kb.data(), n_, devices.empty() ? nullptr : devices.data(), nd, check ? BGLS_KEYS_CHECK : 0u, &h_) == 0;
  }
  ~KeySet() { if (ok_) bgls_keys_free(h_); }
  KeySet(const KeySet&) = delete;
  KeySet& operator=(const KeySet&) = delete;
  bool ok() const { return ok_; }
  // A key set from compressed keys (Point.Marshal encodings, concatenated), decoded and validated on the device(s) in one pass as UnmarshalG2
  // does (bgls_keys_upload_compressed).  !ok() where a key was refused; *first_bad then holds the smallest refused index.
  static std::unique_ptr<KeySet> FromCompressed(const CurveSystem* curve, const Bytes& keys, const std::vector<int>& devices = {}, bool prepare = false,
                                                size_t* first_bad = nullptr) {
    std::unique_ptr<KeySet> ks(new KeySet(curve));
    const size_t cb = bgls_g2_size(curve->id) / 2;
    if (cb == 0 || keys.size() % cb) return ks;
    ks->n_ = keys.size() / cb;
    const int nd = devices.empty() ? 1 : (int)devices.size();
    ks->ok_ = bgls_keys_upload_compressed(curve->id, keys.data(), ks->n_, devices.empty() ? nullptr : devices.data(), nd, prepare ? BGLS_KEYS_PREPARE : 0u, &ks->h_,
                                          first_bad) == 0;
    return ks;
  }
  // the resident keys as Points, read back from the device(s) (bgls_keys_read); empty on failure
  std::vector<Point> Read() const {
    std::vector<Point> out;
    if (!ok_) return out;
    const size_t gb = bgls_g2_size(curve_->id);
    Bytes raw(n_ * gb + 1);
    if (bgls_keys_read(h_, 0, n_, raw.data()) != 0) return out;
    for (size_t i = 0; i < n_; ++i) out.push_back(Point{curve_, BGLS_G2, Bytes(raw.begin() + i * gb, raw.begin() + (i + 1) * gb)});
    return out;
  }
  // verifyAggSig (bgls/bgls.go:94-119) / verifyMultiSignature (bgls/bgls.go:89-92) against the resident keys
  bool VerifyAggregateSignature(const Point& aggsig, const std::vector<Bytes>& msgs, bool allowDuplicates = false) const {
    if (!ok_ || msgs.size() != n_ || aggsig.curve != curve_ || aggsig.group != BGLS_G1) return false;
    Bytes blob;
    std::vector<uint64_t> off(msgs.size() + 1, 0);
    for (size_t i = 0; i < msgs.size(); ++i) {
      blob.insert(blob.end(), msgs[i].begin(), msgs[i].end());
      off[i + 1] = blob.size();
    }
    return bgls_verify_aggregate_h(h_, aggsig.raw.data(), blob.data(), off.data(), n_, allowDuplicates ? 1 : 0) == 1;
  }
  bool VerifyMultiSignature(const Point& aggsig, const Bytes& msg) const {
    if (!ok_ || aggsig.curve != curve_ || aggsig.group != BGLS_G1) return false;
    return bgls_verify_multi_h(h_, aggsig.raw.data(), msg.data(), msg.size()) == 1;
  }
  // DistinctMsgVerifyAggregateSignature (bgls/blsDistinctMessage.go:45-57) against the resident keys, whose wire bytes go in front of the
  // messages on the device
  bool DistinctMsgVerifyAggregateSignature(const Point& aggsig, const std::vector<Bytes>& msgs) const {
    if (!ok_ || msgs.size() != n_ || aggsig.curve != curve_ || aggsig.group != BGLS_G1) return false;
    Bytes blob;
    std::vector<uint64_t> off(msgs.size() + 1, 0);
    for (size_t i = 0; i < msgs.size(); ++i) {
      blob.insert(blob.end(), msgs[i].begin(), msgs[i].end());
      off[i + 1] = blob.size();
    }
    return bgls_verify_aggregate_distinct_h(h_, aggsig.raw.data(), blob.data(), off.data(), n_, nullptr) == 1;
  }
  // ---- sub-slices of the resident keys: MultiSig{keys, sig, msg} (bgls/blsKosk.go:108-112) over registered keys is one subset ----
  // A subset is a list of key indices (each below size(); a repeated index counts once).  One bgls_*_subsets_h call per list of subsets.
  size_t size() const { return n_; }
  // AggregateKeys (bgls/bgls.go:129-131) over every subset: one G2 point per subset; empty on an index outside the set or a failed call
  std::vector<Point> AggregateKeysBySubset(const std::vector<std::vector<size_t>>& subsets) const {
    std::vector<Point> out;
    Bytes rows;
    if (!ok_ || subsets.empty() || !subset_rows(subsets, rows)) return out;
    const size_t pb = curve_->size(BGLS_G2);
    Bytes sums(subsets.size() * pb);
    if (bgls_aggregate_subsets_h(h_, rows.data(), stride(), subsets.size(), sums.data()) != 0) return out;
    for (size_t b = 0; b < subsets.size(); ++b) out.push_back(Point{curve_, BGLS_G2, Bytes(sums.begin() + b * pb, sums.begin() + (b + 1) * pb)});
    return out;
  }
  // aggsigs.size() independent verifyMultiSignature calls (bgls/bgls.go:89-92), set b signed by subset b: one bool per set.  A nil or foreign
  // signature is false without a call; a call that fails as a whole (an off-curve signature, an exhausted hash) is settled set by set.
  std::vector<bool> VerifyMultiSignaturesBySubset(const std::vector<Point>& aggsigs, const std::vector<std::vector<size_t>>& subsets,
                                                  const std::vector<Bytes>& msgs) const {
    std::vector<bool> out(aggsigs.size(), false);
    if (!ok_ || aggsigs.size() != subsets.size() || aggsigs.size() != msgs.size()) return out;
    std::vector<size_t> batch;
    for (size_t b = 0; b < aggsigs.size(); ++b)
      if (aggsigs[b].curve == curve_ && aggsigs[b].group == BGLS_G1) batch.push_back(b);
    auto call = [&](const std::vector<size_t>& idx, std::vector<uint8_t>& verdicts) {
      std::vector<std::vector<size_t>> subs;
      Bytes sb, blob, rows;
      std::vector<uint64_t> off(idx.size() + 1, 0);
      for (size_t i = 0; i < idx.size(); ++i) {
        const size_t b = idx[i];
        subs.push_back(subsets[b]);
        sb.insert(sb.end(), aggsigs[b].raw.begin(), aggsigs[b].raw.end());
        blob.insert(blob.end(), msgs[b].begin(), msgs[b].end());
        off[i + 1] = blob.size();
      }
      if (!subset_rows(subs, rows)) return -1;
      blob.push_back(0);                                   // never an empty array
      verdicts.assign(idx.size(), 0);
      return bgls_verify_multi_subsets_h(h_, sb.data(), rows.data(), stride(), idx.size(), blob.data(), off.data(), verdicts.data(), nullptr, nullptr);
    };
    if (batch.empty()) return out;
    std::vector<uint8_t> verdicts;
    const int rc = call(batch, verdicts);
    for (size_t i = 0; i < batch.size(); ++i) {
      if (rc >= 0) {
        out[batch[i]] = verdicts[i] == 1;
      } else {
        std::vector<uint8_t> v1;
        out[batch[i]] = call({batch[i]}, v1) >= 0 && v1[0] == 1;
      }
    }
    return out;
  }
  // the same for KoskVerifyMultiSignature (bgls/blsKosk.go:117-120): 0x01 prepended to every message
  std::vector<bool> KoskVerifyMultiSignaturesBySubset(const std::vector<Point>& aggsigs, const std::vector<std::vector<size_t>>& subsets,
                                                      const std::vector<Bytes>& msgs) const {
    std::vector<Bytes> ms;
    for (const Bytes& m : msgs) {
      Bytes p(1, 1);
      p.insert(p.end(), m.begin(), m.end());
      ms.push_back(p);
    }
    return VerifyMultiSignaturesBySubset(aggsigs, subsets, ms);
  }
  // verifyAggSig with allowDuplicates = true (bgls/blsKosk.go:100-106) over the sub-slice `subset` of the resident keys, with one hash and
  // one pairing per DISTINCT message (bgls_verify_aggregate_grouped_h): msgs[j] is the message of key subset[j], in the order given (the
  // call wants ascending key order: reordered here).  all = true: every key, msgs[i] the message of key i, subset ignored.  A repeated
  // or foreign index, a length mismatch and every failure of the call are false.
  bool VerifyAggregateSignatureGroupedBySubset(const Point& aggsig, const std::vector<size_t>& subset, const std::vector<Bytes>& msgs,
                                               size_t* n_groups = nullptr, bool all = false) const {
    if (!ok_ || aggsig.curve != curve_ || aggsig.group != BGLS_G1) return false;
    std::vector<size_t> order(msgs.size());
    Bytes row;
    if (all) {
      if (msgs.size() != n_) return false;
      for (size_t j = 0; j < order.size(); ++j) order[j] = j;
    } else {
      if (subset.size() != msgs.size()) return false;
      std::vector<long long> at(n_, -1);
      row.assign(stride(), 0);
      for (size_t j = 0; j < subset.size(); ++j) {
        if (subset[j] >= n_ || at[subset[j]] >= 0) return false;
        at[subset[j]] = (long long)j;
        row[subset[j] >> 3] |= (uint8_t)(1u << (subset[j] & 7));
      }
      size_t k = 0;
      for (size_t i = 0; i < n_; ++i)
        if (at[i] >= 0) order[k++] = (size_t)at[i];
    }
    Bytes blob;
    std::vector<uint64_t> off(msgs.size() + 1, 0);
    for (size_t j = 0; j < order.size(); ++j) {
      blob.insert(blob.end(), msgs[order[j]].begin(), msgs[order[j]].end());
      off[j + 1] = blob.size();
    }
    blob.push_back(0);                                     // never an empty array
    return bgls_verify_aggregate_grouped_h(h_, aggsig.raw.data(), all ? nullptr : row.data(), row.size(), blob.data(), off.data(), msgs.size(), n_groups,
                                           nullptr) == 1;
  }
  // the same for KoskVerifyAggregateSignature: 0x01 prepended to every message
  bool KoskVerifyAggregateSignatureGroupedBySubset(const Point& aggsig, const std::vector<size_t>& subset, const std::vector<Bytes>& msgs,
                                                   size_t* n_groups = nullptr, bool all = false) const {
    std::vector<Bytes> ms;
    for (const Bytes& m : msgs) {
      Bytes p(1, 1);
      p.insert(p.end(), m.begin(), m.end());
      ms.push_back(p);
    }
    return VerifyAggregateSignatureGroupedBySubset(aggsig, subset, ms, n_groups, all);
  }

 private:
  explicit KeySet(const CurveSystem* curve) : curve_(curve), n_(0) {}       // FromCompressed fills it
  size_t stride() const { return n_ / 8 + 1; }             // at least ceil(n / 8), never 0
  // bitmap rows of the subsets (key i of a row: bit i & 7 of byte i >> 3); false on an index outside the set
  bool subset_rows(const std::vector<std::vector<size_t>>& subsets, Bytes& rows) const {
    rows.assign(subsets.size() * stride(), 0);
    for (size_t b = 0; b < subsets.size(); ++b)
      for (size_t i : subsets[b]) {
        if (i >= n_) return false;
        rows[b * stride() + (i >> 3)] |= (uint8_t)(1u << (i & 7));
      }
    return true;
  }

  const CurveSystem* curve_;
  size_t n_;
  bgls_keys_t h_ = 0;
  bool ok_ = false;
};

// ---- hashed aggregation exponents (bgls/blsHAE.go) and multiplicities (bgls/blsKosk.go:137-150) ----
namespace detail {
inline bool g2_bytes(const CurveSystem* curve, const std::vector<Point>& keys, Bytes& kb) {
  for (const Point& k : keys) {
    if (k.curve != curve || k.group != BGLS_G2) return false;
    kb.insert(kb.end(), k.raw.begin(), k.raw.end());
  }
  return true;
}
}  // namespace detail
// hashPubKeysToExponents, bgls/blsHAE.go:80-93: n exponents as 16-byte big-endian strings
inline std::vector<Bytes> hashPubKeysToExponents(const std::vector<Point>& pubkeys) {
  std::vector<Bytes> t;
  if (pubkeys.empty()) return t;
  Bytes kb, out(16 * pubkeys.size());
  if (!detail::g2_bytes(pubkeys[0].curve, pubkeys, kb)) return t;
  if (bgls_hae_exponents(pubkeys[0].curve->id, kb.data(), pubkeys.size(), out.data()) != 0) return t;
  for (size_t i = 0; i < pubkeys.size(); ++i) t.emplace_back(out.begin() + 16 * i, out.begin() + 16 * (i + 1));
  return t;
}
// AggregateSignaturesWithHAE, bgls/blsHAE.go:39-46 (invalid Point = nil on a length mismatch)
inline Point AggregateSignaturesWithHAE(const std::vector<Point>& sigs, const std::vector<Point>& pubkeys) {
  if (sigs.size() != pubkeys.size() || sigs.empty()) return Point{};
  const CurveSystem* curve = sigs[0].curve;
  Bytes sb, kb;
  for (const Point& s : sigs) {
    if (s.curve != curve || s.group != BGLS_G1) return Point{};
    sb.insert(sb.end(), s.raw.begin(), s.raw.end());
  }
  if (!detail::g2_bytes(curve, pubkeys, kb)) return Point{};
  Bytes out(curve->size(BGLS_G1));
  if (bgls_aggregate_signatures_hae(curve->id, sb.data(), kb.data(), sigs.size(), out.data()) != 0) return Point{};
  return Point{curve, BGLS_G1, out};
}
// VerifyAggregateSignatureWithHAE, bgls/blsHAE.go:49-53
inline bool VerifyAggregateSignatureWithHAE(const CurveSystem* curve, const Point& aggsig, const std::vector<Point>& pubkeys,
                                            const std::vector<Bytes>& msgs) {
  if (pubkeys.size() != msgs.size() || aggsig.curve != curve || aggsig.group != BGLS_G1) return false;
  Bytes kb, blob;
  if (!detail::g2_bytes(curve, pubkeys, kb)) return false;
  std::vector<uint64_t> off(msgs.size() + 1, 0);
  for (size_t i = 0; i < msgs.size(); ++i) {
    blob.insert(blob.end(), msgs[i].begin(), msgs[i].end());
    off[i + 1] = blob.size();
  }
  return bgls_verify_aggregate_hae(curve->id, aggsig.raw.data(), kb.data(), blob.data(), off.data(), msgs.size()) == 1;
}
// VerifyMultiSignatureWithHAE, bgls/blsHAE.go:56-58
inline bool VerifyMultiSignatureWithHAE(const CurveSystem* curve, const Point& aggsig, const std::vector<Point>& pubkeys, const Bytes& msg) {
  Bytes kb;
  if (aggsig.curve != curve || aggsig.group != BGLS_G1 || !detail::g2_bytes(curve, pubkeys, kb)) return false;
  return bgls_verify_multi_hae(curve->id, aggsig.raw.data(), kb.data(), pubkeys.size(), msg.data(), msg.size()) == 1;
}
// B independent verifyAggSig calls in ONE bgls_verify_aggregate_batch call: one bool per instance.  An instance that is not made of this
// curve's points (or whose lengths differ) gets verifyAggSig's answer alone; a call that fails as a whole (an encoding or hashing error
// somewhere in the batch) is settled instance by instance, so that the list equals the single calls' results.
inline std::vector<bool> verifyAggSigs(const CurveSystem* curve, const std::vector<Point>& aggsigs, const std::vector<std::vector<Point>>& keys,
                                       const std::vector<std::vector<Bytes>>& msgs, bool allowDuplicates) {
  std::vector<bool> out(aggsigs.size(), false);
  if (keys.size() != aggsigs.size() || msgs.size() != aggsigs.size()) return out;
  std::vector<size_t> batch;
  Bytes sb, kb, blob;
  std::vector<uint64_t> ioff(1, 0), moff(1, 0);
  for (size_t b = 0; b < aggsigs.size(); ++b) {
    Bytes one;
    if (aggsigs[b].curve != curve || aggsigs[b].group != BGLS_G1 || keys[b].size() != msgs[b].size() || !detail::g2_bytes(curve, keys[b], one)) {
      out[b] = verifyAggSig(curve, aggsigs[b], keys[b], msgs[b], allowDuplicates);
      continue;
    }
    batch.push_back(b);
    sb.insert(sb.end(), aggsigs[b].raw.begin(), aggsigs[b].raw.end());
    kb.insert(kb.end(), one.begin(), one.end());
    ioff.push_back(ioff.back() + keys[b].size());
    for (const Bytes& m : msgs[b]) {
      blob.insert(blob.end(), m.begin(), m.end());
      moff.push_back(blob.size());
    }
  }
  if (batch.empty()) return out;
  std::vector<uint8_t> verdicts(batch.size(), 0);
  const int rc = bgls_verify_aggregate_batch(curve->id, sb.data(), kb.data(), ioff.data(), batch.size(), blob.data(), moff.data(), allowDuplicates ? 1 : 0,
                                             verdicts.data(), nullptr);
  for (size_t i = 0; i < batch.size(); ++i) {
    const size_t b = batch[i];
    out[b] = rc >= 0 ? verdicts[i] == 1 : verifyAggSig(curve, aggsigs[b], keys[b], msgs[b], allowDuplicates);
  }
  return out;
}
// B independent VerifyAggregateSignature calls (bgls/bgls.go:82-84) in one batch
inline std::vector<bool> VerifyAggregateSignatures(const CurveSystem* curve, const std::vector<Point>& aggsigs, const std::vector<std::vector<Point>>& keys,
                                                   const std::vector<std::vector<Bytes>>& msgs) {
  return verifyAggSigs(curve, aggsigs, keys, msgs, false);
}
// B independent KoskVerifyAggregateSignature calls (bgls/blsKosk.go:100-106): 0x01 prepended to every message, duplicates allowed
inline std::vector<bool> KoskVerifyAggregateSignatures(const CurveSystem* curve, const std::vector<Point>& aggsigs,
                                                       const std::vector<std::vector<Point>>& keys, const std::vector<std::vector<Bytes>>& msgs) {
  std::vector<std::vector<Bytes>> pm(msgs.size());
  for (size_t b = 0; b < msgs.size(); ++b)
    for (const Bytes& m : msgs[b]) {
      Bytes one(1, 1);
      one.insert(one.end(), m.begin(), m.end());
      pm[b].push_back(one);
    }
  return verifyAggSigs(curve, aggsigs, keys, pm, true);
}
// B independent verifyMultiSignature calls (bgls/bgls.go:89-92) in ONE bgls_verify_multi_sets call: one bool per set.  A set that is not
// made of this curve's points gets verifyMultiSignature's answer alone; a call that fails as a whole (an encoding or hashing error
// somewhere in the batch) is settled set by set, so that the list equals the single calls' results.
inline std::vector<bool> verifyMultiSignatures(const CurveSystem* curve, const std::vector<Point>& aggsigs, const std::vector<std::vector<Point>>& keys,
                                               const std::vector<Bytes>& msgs) {
  std::vector<bool> out(aggsigs.size(), false);
  if (keys.size() != aggsigs.size() || msgs.size() != aggsigs.size()) return out;
  std::vector<size_t> batch;
  Bytes sb, kb, blob;
  std::vector<uint64_t> koff(1, 0), moff(1, 0);
  for (size_t b = 0; b < aggsigs.size(); ++b) {
    Bytes one;
    if (aggsigs[b].curve != curve || aggsigs[b].group != BGLS_G1 || !detail::g2_bytes(curve, keys[b], one)) {
      out[b] = verifyMultiSignature(curve, aggsigs[b], keys[b], msgs[b]);
      continue;
    }
    batch.push_back(b);
    sb.insert(sb.end(), aggsigs[b].raw.begin(), aggsigs[b].raw.end());
    kb.insert(kb.end(), one.begin(), one.end());
    koff.push_back(koff.back() + keys[b].size());
    blob.insert(blob.end(), msgs[b].begin(), msgs[b].end());
    moff.push_back(blob.size());
  }
  if (batch.empty()) return out;
  std::vector<uint8_t> verdicts(batch.size(), 0);
  const int rc = bgls_verify_multi_sets(curve->id, sb.data(), kb.data(), koff.data(), batch.size(), blob.data(), moff.data(), verdicts.data(), nullptr);
  for (size_t i = 0; i < batch.size(); ++i) {
    const size_t b = batch[i];
    out[b] = rc >= 0 ? verdicts[i] == 1 : verifyMultiSignature(curve, aggsigs[b], keys[b], msgs[b]);
  }
  return out;
}
// "Are these multi-signatures all valid?" under one combined check per group of consecutive sets (bgls_verify_multi_sets_combined: one
// final exponentiation per group).  group: sets per group, 0 = one group over all sets.  seed: 32 bytes from a CSPRNG drawn AFTER the
// inputs are fixed (empty: drawn from std::random_device here).  One bool per group; ok (nullable) is cleared when the call could not
// run -- lengths that differ, a set not made of this curve's points, an encoding or hashing error anywhere -- and the list is then all false.
inline std::vector<bool> VerifyMultiSignaturesCombined(const CurveSystem* curve, const std::vector<Point>& aggsigs, const std::vector<std::vector<Point>>& keys,
                                                       const std::vector<Bytes>& msgs, size_t group = 0, Bytes seed = Bytes(), bool* ok = nullptr) {
  const size_t n = aggsigs.size();
  std::vector<uint64_t> goff(1, 0);
  for (size_t at = 0; at < n;) goff.push_back(at = (group && at + group < n) ? at + group : n);
  std::vector<bool> out(goff.size() - 1, false);
  if (ok) *ok = false;
  if (keys.size() != n || msgs.size() != n || (!seed.empty() && seed.size() != 32)) return out;
  if (seed.empty()) {
    std::random_device rd;
    for (int i = 0; i < 32; ++i) seed.push_back((uint8_t)rd());
  }
  Bytes sb, kb, blob;
  std::vector<uint64_t> koff(1, 0), moff(1, 0);
  for (size_t b = 0; b < n; ++b) {
    Bytes one;
    if (aggsigs[b].curve != curve || aggsigs[b].group != BGLS_G1 || !detail::g2_bytes(curve, keys[b], one)) return out;
    sb.insert(sb.end(), aggsigs[b].raw.begin(), aggsigs[b].raw.end());
    kb.insert(kb.end(), one.begin(), one.end());
    koff.push_back(koff.back() + keys[b].size());
    blob.insert(blob.end(), msgs[b].begin(), msgs[b].end());
    moff.push_back(blob.size());
  }
  if (ok) *ok = true;
  if (n == 0) return out;
  std::vector<uint8_t> verdicts(out.size(), 0);
  const int rc = bgls_verify_multi_sets_combined(curve->id, sb.data(), kb.data(), koff.data(), n, blob.data(), moff.data(), goff.data(), out.size(), seed.data(),
                                                 verdicts.data(), nullptr);
  if (rc < 0 && ok) *ok = false;
  for (size_t g = 0; g < out.size(); ++g) out[g] = rc >= 0 && verdicts[g] == 1;
  return out;
}
// the same with 0x01 prepended to every message (bgls/blsKosk.go:117-120)
inline std::vector<bool> KoskVerifyMultiSignaturesCombined(const CurveSystem* curve, const std::vector<Point>& aggsigs, const std::vector<std::vector<Point>>& keys,
                                                           const std::vector<Bytes>& msgs, size_t group = 0, Bytes seed = Bytes(), bool* ok = nullptr) {
  std::vector<Bytes> pm;
  for (const Bytes& m : msgs) {
    Bytes one(1, 1);
    one.insert(one.end(), m.begin(), m.end());
    pm.push_back(one);
  }
  return VerifyMultiSignaturesCombined(curve, aggsigs, keys, pm, group, seed, ok);
}
// One bool per set at the combined check's cost where everything is valid: ONE combined call over groups of `group` sets, then ONE
// verifyMultiSignatures call over only the sets of the rejected groups; the sets of accepted groups get true.  Where the combined call
// cannot run, every set goes through verifyMultiSignatures.
inline std::vector<bool> VerifyMultiSignaturesLocated(const CurveSystem* curve, const std::vector<Point>& aggsigs, const std::vector<std::vector<Point>>& keys,
                                                      const std::vector<Bytes>& msgs, size_t group = 64, Bytes seed = Bytes()) {
  const size_t n = aggsigs.size();
  bool ok = false;
  const std::vector<bool> groups = VerifyMultiSignaturesCombined(curve, aggsigs, keys, msgs, group, seed, &ok);
  if (!ok) return verifyMultiSignatures(curve, aggsigs, keys, msgs);
  std::vector<bool> out(n, true);
  std::vector<size_t> again;
  for (size_t g = 0; g < groups.size(); ++g)
    if (!groups[g])
      for (size_t b = g * (group ? group : n); b < n && (group == 0 || b < (g + 1) * group); ++b) again.push_back(b);
  if (again.empty()) return out;
  std::vector<Point> s2;
  std::vector<std::vector<Point>> k2;
  std::vector<Bytes> m2;
  for (size_t b : again) { s2.push_back(aggsigs[b]); k2.push_back(keys[b]); m2.push_back(msgs[b]); }
  const std::vector<bool> v = verifyMultiSignatures(curve, s2, k2, m2);
  for (size_t i = 0; i < again.size(); ++i) out[again[i]] = v[i];
  return out;
}
// B independent VerifyMultiSignatureWithHAE calls (bgls/blsHAE.go:56-58) in ONE bgls_verify_multi_hae_sets call: one bool per set.  A set
// that is not made of this curve's points gets VerifyMultiSignatureWithHAE's answer alone; a call that fails as a whole is settled set by set.
inline std::vector<bool> VerifyMultiSignaturesWithHAE(const CurveSystem* curve, const std::vector<Point>& aggsigs, const std::vector<std::vector<Point>>& keys,
                                                      const std::vector<Bytes>& msgs) {
  std::vector<bool> out(aggsigs.size(), false);
  if (keys.size() != aggsigs.size() || msgs.size() != aggsigs.size()) return out;
  std::vector<size_t> batch;
  Bytes sb, kb, blob;
  std::vector<uint64_t> koff(1, 0), moff(1, 0);
  for (size_t b = 0; b < aggsigs.size(); ++b) {
    Bytes one;
    if (aggsigs[b].curve != curve || aggsigs[b].group != BGLS_G1 || !detail::g2_bytes(curve, keys[b], one)) {
      out[b] = VerifyMultiSignatureWithHAE(curve, aggsigs[b], keys[b], msgs[b]);
      continue;
    }
    batch.push_back(b);
    sb.insert(sb.end(), aggsigs[b].raw.begin(), aggsigs[b].raw.end());
    kb.insert(kb.end(), one.begin(), one.end());
    koff.push_back(koff.back() + keys[b].size());
    blob.insert(blob.end(), msgs[b].begin(), msgs[b].end());
    moff.push_back(blob.size());
  }
  if (batch.empty()) return out;
  std::vector<uint8_t> verdicts(batch.size(), 0);
  const int rc = bgls_verify_multi_hae_sets(curve->id, sb.data(), kb.data(), koff.data(), batch.size(), blob.data(), moff.data(), verdicts.data(), nullptr,
                                            nullptr);
  for (size_t i = 0; i < batch.size(); ++i) {
    const size_t b = batch[i];
    out[b] = rc >= 0 ? verdicts[i] == 1 : VerifyMultiSignatureWithHAE(curve, aggsigs[b], keys[b], msgs[b]);
  }
  return out;
}
// B independent KoskVerifyMultiSignature calls (bgls/blsKosk.go:117-120): 0x01 prepended to every message
inline std::vector<bool> KoskVerifyMultiSignatures(const CurveSystem* curve, const std::vector<Point>& aggsigs, const std::vector<std::vector<Point>>& keys,
                                                   const std::vector<Bytes>& msgs) {
  std::vector<Bytes> pm;
  for (const Bytes& m : msgs) {
    Bytes one(1, 1);
    one.insert(one.end(), m.begin(), m.end());
    pm.push_back(one);
  }
  return verifyMultiSignatures(curve, aggsigs, keys, pm);
}
// B independent VerifySingleSignature calls (bgls/bgls.go:59-70): one key per set
inline std::vector<bool> VerifySingleSignatures(const CurveSystem* curve, const std::vector<Point>& sigs, const std::vector<Point>& pubKeys,
                                                const std::vector<Bytes>& msgs) {
  std::vector<std::vector<Point>> keys;
  for (const Point& k : pubKeys) keys.push_back({k});
  return verifyMultiSignatures(curve, sigs, keys, msgs);
}
// B independent KoskVerifySingleSignature calls (bgls/blsKosk.go:86-90)
inline std::vector<bool> KoskVerifySingleSignatures(const CurveSystem* curve, const std::vector<Point>& sigs, const std::vector<Point>& pubKeys,
                                                    const std::vector<Bytes>& msgs) {
  std::vector<std::vector<Point>> keys;
  for (const Point& k : pubKeys) keys.push_back({k});
  return KoskVerifyMultiSignatures(curve, sigs, keys, msgs);
}
// ---- distinct messages (bgls/blsDistinctMessage.go) and key registration (bgls/blsKosk.go:44-69): the message that is hashed is derived
// from the signer's key, and the library derives it on the device -- nothing is prefixed here ----
// DistinctMsgSign, bgls/blsDistinctMessage.go:23-34
inline Point DistinctMsgSign(const CurveSystem* curve, const Bytes& sk_be32, const Bytes& msg) {
  std::vector<Bytes> one(1, msg);
  std::vector<Point> h = curve->HashToG1Keyed({LoadPublicKey(curve, sk_be32)}, &one);
  return h.empty() ? Point{} : h[0].Mul(sk_be32);
}
// Authenticate, bgls/blsKosk.go:44-55: a signature on the marshalled key
inline Point Authenticate(const CurveSystem* curve, const Bytes& sk_be32) {
  std::vector<Point> h = curve->HashToG1Keyed({LoadPublicKey(curve, sk_be32)});
  return h.empty() ? Point{} : h[0].Mul(sk_be32);
}
// DistinctMsgVerifyAggregateSignature, bgls/blsDistinctMessage.go:45-57
inline bool DistinctMsgVerifyAggregateSignature(const CurveSystem* curve, const Point& aggsig, const std::vector<Point>& keys, const std::vector<Bytes>& msgs) {
  if (keys.size() != msgs.size() || aggsig.curve != curve || aggsig.group != BGLS_G1) return false;
  Bytes kb, blob;
  if (!detail::g2_bytes(curve, keys, kb)) return false;
  std::vector<uint64_t> off(msgs.size() + 1, 0);
  for (size_t i = 0; i < msgs.size(); ++i) {
    blob.insert(blob.end(), msgs[i].begin(), msgs[i].end());
    off[i + 1] = blob.size();
  }
  return bgls_verify_aggregate_distinct(curve->id, aggsig.raw.data(), kb.data(), blob.data(), off.data(), keys.size()) == 1;
}
// B independent DistinctMsgVerifyAggregateSignature calls in ONE bgls_verify_aggregate_distinct_batch call, with verifyAggSigs' conventions
inline std::vector<bool> DistinctMsgVerifyAggregateSignatures(const CurveSystem* curve, const std::vector<Point>& aggsigs,
                                                              const std::vector<std::vector<Point>>& keys, const std::vector<std::vector<Bytes>>& msgs) {
  std::vector<bool> out(aggsigs.size(), false);
  if (keys.size() != aggsigs.size() || msgs.size() != aggsigs.size()) return out;
  std::vector<size_t> batch;
  Bytes sb, kb, blob;
  std::vector<uint64_t> ioff(1, 0), moff(1, 0);
  for (size_t b = 0; b < aggsigs.size(); ++b) {
    Bytes one;
    if (aggsigs[b].curve != curve || aggsigs[b].group != BGLS_G1 || keys[b].size() != msgs[b].size() || !detail::g2_bytes(curve, keys[b], one)) continue;
    batch.push_back(b);
    sb.insert(sb.end(), aggsigs[b].raw.begin(), aggsigs[b].raw.end());
    kb.insert(kb.end(), one.begin(), one.end());
    ioff.push_back(ioff.back() + keys[b].size());
    for (const Bytes& m : msgs[b]) {
      blob.insert(blob.end(), m.begin(), m.end());
      moff.push_back(blob.size());
    }
  }
  if (batch.empty()) return out;
  std::vector<uint8_t> verdicts(batch.size(), 0);
  const int rc = bgls_verify_aggregate_distinct_batch(curve->id, sb.data(), kb.data(), ioff.data(), batch.size(), blob.data(), moff.data(), verdicts.data(),
                                                      nullptr);
  for (size_t i = 0; i < batch.size(); ++i) {
    const size_t b = batch[i];
    out[b] = rc >= 0 ? verdicts[i] == 1 : DistinctMsgVerifyAggregateSignature(curve, aggsigs[b], keys[b], msgs[b]);
  }
  return out;
}
namespace detail {
// the items made of this curve's points through ONE bgls_verify_single_distinct_batch (msgs given) or bgls_check_authentication_batch
// call; any other item is false, and a call that fails as a whole is settled item by item through batches of one
inline std::vector<bool> verify_single_keyed(const CurveSystem* curve, const std::vector<Point>& sigs, const std::vector<Point>& pubKeys,
                                             const std::vector<Bytes>* msgs) {
  const size_t n = sigs.size();
  std::vector<bool> out(n, false);
  if (pubKeys.size() != n || (msgs && msgs->size() != n)) return out;
  std::vector<size_t> batch;
  Bytes sb, kb, blob;
  std::vector<uint64_t> moff(1, 0);
  for (size_t b = 0; b < n; ++b) {
    if (sigs[b].curve != curve || sigs[b].group != BGLS_G1 || pubKeys[b].curve != curve || pubKeys[b].group != BGLS_G2) continue;
    batch.push_back(b);
    sb.insert(sb.end(), sigs[b].raw.begin(), sigs[b].raw.end());
    kb.insert(kb.end(), pubKeys[b].raw.begin(), pubKeys[b].raw.end());
    if (msgs) blob.insert(blob.end(), (*msgs)[b].begin(), (*msgs)[b].end());
    moff.push_back(blob.size());
  }
  if (batch.empty()) return out;
  std::vector<uint8_t> verdicts(batch.size(), 0);
  const int rc = msgs ? bgls_verify_single_distinct_batch(curve->id, sb.data(), kb.data(), blob.data(), moff.data(), batch.size(), verdicts.data(), nullptr)
                      : bgls_check_authentication_batch(curve->id, kb.data(), sb.data(), batch.size(), verdicts.data(), nullptr);
  if (rc < 0 && batch.size() > 1) {
    for (size_t b : batch) {
      const std::vector<Bytes> one(1, msgs ? (*msgs)[b] : Bytes());
      out[b] = verify_single_keyed(curve, {sigs[b]}, {pubKeys[b]}, msgs ? &one : nullptr)[0];
    }
    return out;
  }
  for (size_t i = 0; i < batch.size(); ++i) out[batch[i]] = rc >= 0 && verdicts[i] == 1;
  return out;
}
}  // namespace detail
// B independent DistinctMsgVerifySingleSignature calls (bgls/blsDistinctMessage.go:37-40) in one batch
inline std::vector<bool> DistinctMsgVerifySingleSignatures(const CurveSystem* curve, const std::vector<Point>& sigs, const std::vector<Point>& pubKeys,
                                                           const std::vector<Bytes>& msgs) {
  return detail::verify_single_keyed(curve, sigs, pubKeys, &msgs);
}
inline bool DistinctMsgVerifySingleSignature(const CurveSystem* curve, const Point& sig, const Point& pubKey, const Bytes& msg) {
  return DistinctMsgVerifySingleSignatures(curve, {sig}, {pubKey}, {msg})[0];
}
// B independent CheckAuthentication calls (bgls/blsKosk.go:59-69) in one batch
inline std::vector<bool> CheckAuthentications(const CurveSystem* curve, const std::vector<Point>& pubKeys, const std::vector<Point>& authentications) {
  return detail::verify_single_keyed(curve, authentications, pubKeys, nullptr);
}
inline bool CheckAuthentication(const CurveSystem* curve, const Point& pubKey, const Point& authentication) {
  return CheckAuthentications(curve, {pubKey}, {authentication})[0];
}
// KoskVerifyBatchMultiSignature, bgls/blsKosk.go:126-133: one call -- every key set summed in one launch, ONE aggregate verification
inline bool KoskVerifyBatchMultiSignature(const CurveSystem* curve, const std::vector<Point>& aggsigs, const std::vector<std::vector<Point>>& pubkeys,
                                          const std::vector<Bytes>& msgs) {
  if (aggsigs.size() != pubkeys.size() || pubkeys.size() != msgs.size() || msgs.empty()) return false;
  Bytes sb, kb, blob;
  std::vector<uint64_t> koff(pubkeys.size() + 1, 0), moff(msgs.size() + 1, 0);
  for (size_t i = 0; i < msgs.size(); ++i) {
    if (aggsigs[i].curve != curve || aggsigs[i].group != BGLS_G1) return false;
    sb.insert(sb.end(), aggsigs[i].raw.begin(), aggsigs[i].raw.end());
    Bytes one;
    if (!detail::g2_bytes(curve, pubkeys[i], one)) return false;
    kb.insert(kb.end(), one.begin(), one.end());
    koff[i + 1] = koff[i] + pubkeys[i].size();
    blob.push_back(1);                                   // the Kosk prefix (blsKosk.go:100-106)
    blob.insert(blob.end(), msgs[i].begin(), msgs[i].end());
    moff[i + 1] = blob.size();
  }
  return bgls_verify_multi_batch(curve->id, sb.data(), kb.data(), koff.data(), msgs.size(), blob.data(), moff.data(), 1) == 1;
}
// KoskVerifyMultiSignatureWithMultiplicity, bgls/blsKosk.go:137-150 (multiplicity == nullptr: plain KoskVerifyMultiSignature)
inline bool KoskVerifyMultiSignatureWithMultiplicity(const CurveSystem* curve, const Point& aggsig, const std::vector<Point>& keys,
                                                     const std::vector<int64_t>* multiplicity, const Bytes& msg) {
  if (!multiplicity) return KoskVerifyMultiSignature(curve, aggsig, keys, msg);
  if (keys.size() != multiplicity->size()) return false;
  Bytes kb, m(1, 1);
  if (aggsig.curve != curve || aggsig.group != BGLS_G1 || !detail::g2_bytes(curve, keys, kb)) return false;
  m.insert(m.end(), msg.begin(), msg.end());
  return bgls_verify_multi_multiplicity(curve->id, aggsig.raw.data(), kb.data(), multiplicity->data(), keys.size(), m.data(), m.size()) == 1;
}

}  // namespace bgls_go

// ---- Boneh-Boyen signatures (package bbsigs, bbsigs/bbsigs.go) ----
// bgls::bb_verify_batch: n independent bbsigs.Verify calls (bbsigs/bbsigs.go:68-73) in ONE bgls_bb_verify_batch call, one bool per
// item.  Item b is the signature (sigmas[b], rs[b]) on the message scalar ms[b] under the key (us[b], vs[b]); scalars are 32-byte
// big-endian magnitudes, used as given (reduce negative or larger big.Ints modulo the order first, as the Python mirror does).  An
// item that is not made of this curve's points, or whose scalars are not 32 bytes, is rejected; a call that fails as a whole (an
// encoding error somewhere in the batch) is settled item by item.  (A function in namespace bgls: the header's public name for the
// call, next to the Go-named mirror bgls_go.)
namespace bgls {
inline std::vector<bool> bb_verify_batch(const curves::CurveSystem* curve, const std::vector<curves::Point>& sigmas, const std::vector<curves::Bytes>& rs,
                                         const std::vector<curves::Point>& us, const std::vector<curves::Point>& vs, const std::vector<curves::Bytes>& ms) {
  const size_t n = sigmas.size();
  std::vector<bool> out(n, false);
  if (rs.size() != n || us.size() != n || vs.size() != n || ms.size() != n) return out;
  std::vector<size_t> batch;
  curves::Bytes sb, rb, kb, mb;
  for (size_t b = 0; b < n; ++b) {
    if (sigmas[b].curve != curve || sigmas[b].group != BGLS_G1 || us[b].curve != curve || us[b].group != BGLS_G2 || vs[b].curve != curve ||
        vs[b].group != BGLS_G2 || rs[b].size() != 32 || ms[b].size() != 32)
      continue;
    batch.push_back(b);
    sb.insert(sb.end(), sigmas[b].raw.begin(), sigmas[b].raw.end());
    rb.insert(rb.end(), rs[b].begin(), rs[b].end());
    kb.insert(kb.end(), us[b].raw.begin(), us[b].raw.end());
    kb.insert(kb.end(), vs[b].raw.begin(), vs[b].raw.end());
    mb.insert(mb.end(), ms[b].begin(), ms[b].end());
  }
  if (batch.empty()) return out;
  std::vector<uint8_t> verdicts(batch.size(), 0);
  const int rc = bgls_bb_verify_batch(curve->id, sb.data(), rb.data(), kb.data(), mb.data(), batch.size(), verdicts.data(), nullptr);
  if (rc < 0 && batch.size() > 1) {
    for (size_t b : batch) out[b] = bb_verify_batch(curve, {sigmas[b]}, {rs[b]}, {us[b]}, {vs[b]}, {ms[b]})[0];
    return out;
  }
  for (size_t i = 0; i < batch.size(); ++i) out[batch[i]] = rc >= 0 && verdicts[i] == 1;
  return out;
}
// "Are these Boneh-Boyen signatures all valid?" under one combined check per group of consecutive items (bgls_bb_verify_batch_combined:
// shared squarings and one final exponentiation per group).  group: items per group, 0 = one group over all items.  seed: 32 bytes from
// a CSPRNG drawn AFTER the inputs are fixed (empty: drawn from std::random_device here).  One bool per group; ok (nullable) is cleared
// when the call could not run -- lengths that differ, an item not made of this curve's points or of 32-byte scalars, an encoding error
// anywhere -- and the list is then all false.
inline std::vector<bool> bb_verify_batch_combined(const curves::CurveSystem* curve, const std::vector<curves::Point>& sigmas, const std::vector<curves::Bytes>& rs,
                                                  const std::vector<curves::Point>& us, const std::vector<curves::Point>& vs, const std::vector<curves::Bytes>& ms,
                                                  size_t group = 0, curves::Bytes seed = curves::Bytes(), bool* ok = nullptr) {
  const size_t n = sigmas.size();
  std::vector<uint64_t> goff(1, 0);
  for (size_t at = 0; at < n;) goff.push_back(at = (group && at + group < n) ? at + group : n);
  std::vector<bool> out(goff.size() - 1, false);
  if (ok) *ok = false;
  if (rs.size() != n || us.size() != n || vs.size() != n || ms.size() != n || (!seed.empty() && seed.size() != 32)) return out;
  if (seed.empty()) {
    std::random_device rd;
    for (int i = 0; i < 32; ++i) seed.push_back((uint8_t)rd());
  }
  curves::Bytes sb, rb, kb, mb;
  for (size_t b = 0; b < n; ++b) {
    if (sigmas[b].curve != curve || sigmas[b].group != BGLS_G1 || us[b].curve != curve || us[b].group != BGLS_G2 || vs[b].curve != curve ||
        vs[b].group != BGLS_G2 || rs[b].size() != 32 || ms[b].size() != 32)
      return out;
    sb.insert(sb.end(), sigmas[b].raw.begin(), sigmas[b].raw.end());
    rb.insert(rb.end(), rs[b].begin(), rs[b].end());
    kb.insert(kb.end(), us[b].raw.begin(), us[b].raw.end());
    kb.insert(kb.end(), vs[b].raw.begin(), vs[b].raw.end());
    mb.insert(mb.end(), ms[b].begin(), ms[b].end());
  }
  if (ok) *ok = true;
  if (n == 0) return out;
  std::vector<uint8_t> verdicts(out.size(), 0);
  const int rc = bgls_bb_verify_batch_combined(curve->id, sb.data(), rb.data(), kb.data(), mb.data(), n, goff.data(), out.size(), seed.data(), verdicts.data(),
                                               nullptr);
  if (rc < 0 && ok) *ok = false;
  for (size_t g = 0; g < out.size(); ++g) out[g] = rc >= 0 && verdicts[g] == 1;
  return out;
}
// One bool per item at the combined check's cost where everything is valid: ONE combined call over groups of `group` items, then ONE
// bb_verify_batch call over only the items of the rejected groups; the items of accepted groups get true.  Where the combined call cannot
// run, every item goes through bb_verify_batch.
inline std::vector<bool> bb_verify_batch_located(const curves::CurveSystem* curve, const std::vector<curves::Point>& sigmas, const std::vector<curves::Bytes>& rs,
                                                 const std::vector<curves::Point>& us, const std::vector<curves::Point>& vs, const std::vector<curves::Bytes>& ms,
                                                 size_t group = 64, curves::Bytes seed = curves::Bytes()) {
  const size_t n = sigmas.size();
  bool ok = false;
  const std::vector<bool> groups = bb_verify_batch_combined(curve, sigmas, rs, us, vs, ms, group, seed, &ok);
  if (!ok) return bb_verify_batch(curve, sigmas, rs, us, vs, ms);
  std::vector<bool> out(n, true);
  std::vector<size_t> again;
  for (size_t g = 0; g < groups.size(); ++g)
    if (!groups[g])
      for (size_t b = g * (group ? group : n); b < n && (group == 0 || b < (g + 1) * group); ++b) again.push_back(b);
  if (again.empty()) return out;
  std::vector<curves::Point> s2, u2, v2;
  std::vector<curves::Bytes> r2, m2;
  for (size_t b : again) {
    s2.push_back(sigmas[b]);
    r2.push_back(rs[b]);
    u2.push_back(us[b]);
    v2.push_back(vs[b]);
    m2.push_back(ms[b]);
  }
  const std::vector<bool> settled = bb_verify_batch(curve, s2, r2, u2, v2, m2);
  for (size_t i = 0; i < again.size(); ++i) out[again[i]] = settled[i];
  return out;
}
}  // namespace bgls
