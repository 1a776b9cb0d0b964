// dm_decide_plan.h — what the host decides of a round of requests before anything reaches the
// device (dm_decide.cpp): whether the requests are valid, their stable order by resource, the
// work items of k_decide (dm_round.hip) and of the fast path (dm_decide_fast.hip), the areas
// the fast path's kernels index into, and from those the element count of every device buffer
// of the round (dm_decide_round.h DecideRound holds the buffers).  The kernels trust these
// numbers: an area or a count too small is a write out of bounds.  Plain C++17, no HIP: the
// plan is tested on the CPU (tests/test_decide_plan.py).
#pragma once
#include <algorithm>
#include <cstdint>
#include <unordered_map>
#include <vector>

namespace dm {

struct ReqItem {
  int32_t seg;
  int32_t fast;  // 1 + its slot of the fast path (FastItem), 0: decided by k_decide only
  int64_t qlo, qhi;
  int64_t scr;
};

constexpr int kFdMin = 64;       // requests on one resource before the fast path is tried
constexpr int kFdBlock = 2048;   // requests per Assign-event block (2 events each)
constexpr int kFdRows = 4096;    // rows per workgroup of the fast path's row passes
constexpr int kFdChunk = 1024;   // scan elements per workgroup (4 per thread)
struct FastItem {
  int32_t item;  // index of the resource's ReqItem
  int32_t nblk;  // event blocks: ceil(K / kFdBlock)
  int64_t k0, K; // its requests [k0, k0 + K) of the round (grouped order)
  int64_t m0;    // offset of its sorted-wants area (n + 1 entries)
  int64_t e0;    // offset of its events (2 K)
  int64_t b0;    // first event block (global block index)
  int64_t n;     // rows of the resource
  int64_t c0;    // first row chunk (kFdRows rows each; global chunk index)
  int32_t nch;   // row chunks
  int32_t repeats;  // 1: some row is requested twice (the grants then need the sequential recurrence)
};

// Why a round is rejected: the first failing request in the caller's order decides, its row
// before its subclients (dm_decide turns these into DM_E_RANGE and DM_E_INVAL).
enum class RoundError : uint8_t { none, row_range, subclients };

struct RoundPlan {
  RoundError error = RoundError::none;  // set: nothing below is filled
  int64_t n = 0;               // requests
  std::vector<int64_t> order;  // [n] grouped position -> the caller's index; stable by resource
  // One item per resource with requests, in resource order: its requests [qlo, qhi) of the
  // grouped order and its rows' place [scr, scr + rows) in the round's scratch copy.
  std::vector<ReqItem> items;
  int64_t scratch = 0;  // rows of the scratch copy
  // Resources with many requests try the fast path: per resource its scan / sort areas, per
  // request the previous request of the round on the same row (its Assign is what the row
  // holds then; a grouped index within the resource's own requests, or -1).  The device
  // decides whether the round qualifies (FastRes::ok); k_decide takes every item it does not.
  std::vector<FastItem> fitems;
  std::vector<int64_t> prev;  // [n]; empty in a round without fast items
  int64_t m = 0, e = 0, b = 0, c = 0;  // the areas' totals: sorted wants, events, event blocks, row chunks
  // the event blocks' segments of the pair sort: the b begins, then the b ends (block j of an
  // item: events [e0 + 2 j kFdBlock, e0 + 2 min(K, (j + 1) kFdBlock)))
  std::vector<int64_t> bounds;
  int64_t parts = 0;  // partials of the longest scan (an item's K requests or n + 1 sorted wants)
  bool fast() const { return !fitems.empty(); }
};

// seg_off: the store's R + 1 row offsets, N its rows; rows / subclients: the caller's n
// requests; fast: the fast path's switch (DM_DECIDE_FAST); sub_max: the largest subclients
// value a row holds (kSubMax).
inline RoundPlan plan_round(const int64_t* seg_off, int64_t R, int64_t N, const int64_t* rows,
                            const int64_t* subclients, int64_t n, bool fast, int64_t sub_max) {
  RoundPlan p;
  p.n = n;
  std::vector<int64_t> seg_of((size_t)n);
  for (int64_t k = 0; k < n; ++k) {
    if (rows[k] < 0 || rows[k] >= N) return p.error = RoundError::row_range, p;
    if (subclients[k] < 0 || subclients[k] > sub_max) return p.error = RoundError::subclients, p;
    seg_of[(size_t)k] = std::upper_bound(seg_off, seg_off + R + 1, rows[k]) - seg_off - 1;
  }
  p.order.resize((size_t)n);
  for (int64_t i = 0; i < n; ++i) p.order[(size_t)i] = i;
  std::stable_sort(p.order.begin(), p.order.end(),
                   [&](int64_t a, int64_t b) { return seg_of[(size_t)a] < seg_of[(size_t)b]; });
  for (int64_t i = 0; i < n; ++i) {
    const int64_t seg = seg_of[(size_t)p.order[(size_t)i]];
    if (p.items.empty() || p.items.back().seg != (int32_t)seg) {
      p.items.push_back(ReqItem{(int32_t)seg, 0, i, i, p.scratch});
      p.scratch += seg_off[seg + 1] - seg_off[seg];
    }
    p.items.back().qhi = i + 1;
  }
  int64_t most = 1;
  for (size_t ii = 0; fast && ii < p.items.size(); ++ii) {
    ReqItem& itm = p.items[ii];
    const int64_t K = itm.qhi - itm.qlo;
    if (K < kFdMin) continue;
    if (p.prev.empty()) p.prev.assign((size_t)n, -1);
    FastItem f{};
    f.item = (int32_t)ii;
    f.k0 = itm.qlo;
    f.K = K;
    f.n = seg_off[itm.seg + 1] - seg_off[itm.seg];
    f.nblk = (int32_t)((K + kFdBlock - 1) / kFdBlock);
    f.nch = (int32_t)std::max<int64_t>(1, (f.n + kFdRows - 1) / kFdRows);
    f.m0 = p.m;
    f.e0 = p.e;
    f.b0 = p.b;
    f.c0 = p.c;
    p.m += f.n + 1;
    p.e += 2 * K;
    p.b += f.nblk;
    p.c += f.nch;
    std::unordered_map<int64_t, int64_t> last;
    last.reserve((size_t)(2 * K));
    for (int64_t k = itm.qlo; k < itm.qhi; ++k) {
      const int64_t row = rows[p.order[(size_t)k]];
      auto seen = last.find(row);
      if (seen != last.end()) {
        p.prev[(size_t)k] = seen->second;
        f.repeats = 1;
      }
      last[row] = k;
    }
    itm.fast = (int32_t)p.fitems.size() + 1;
    p.fitems.push_back(f);
    most = std::max(most, std::max(f.K, f.n + 1));
  }
  if (p.fast()) p.parts = (most + kFdChunk - 1) / kFdChunk;
  p.bounds.resize((size_t)(2 * p.b));
  for (const FastItem& f : p.fitems)
    for (int64_t j = 0; j < f.nblk; ++j) {
      p.bounds[(size_t)(f.b0 + j)] = f.e0 + 2 * j * kFdBlock;
      p.bounds[(size_t)(p.b + f.b0 + j)] = f.e0 + 2 * std::min<int64_t>(f.K, (j + 1) * kFdBlock);
    }
  return p;
}

// The round's device buffers (DecideRound's members of the same names, the fields of ReqArgs
// and FastArgs in dm_device.h), and the one rule of how many elements each holds.
enum class RoundBuf : uint8_t {
  // the requests in grouped order, their results, the work items, the scratch copy (ReqArgs)
  rows, has, wants, sub, gets, exp, items, sc_has, sc_wants, sc_sub,
  // the fast path (FastArgs, and the scans' partials and the pair sort's segments beside it)
  res, prev, pw, v, sc, ld, keys, keys_s, ps, ev_in, evs_in, ev, evs, ecnt, esum, bdc, bds, pc, pt, part, bounds
};
constexpr int kRoundBufs = (int)RoundBuf::bounds + 1;

// A round without fast items asks nothing (0) of the fast path's buffers: they stay as an
// earlier round left them.
inline int64_t round_count(const RoundPlan& p, RoundBuf buf) {
  using B = RoundBuf;
  if (buf >= B::res && !p.fast()) return 0;
  switch (buf) {
    case B::rows: case B::has: case B::wants: case B::sub: case B::gets: case B::exp:
    case B::prev: case B::pw: case B::v: case B::sc: case B::ld:
      return p.n;  // [n requests]
    case B::items:
      return (int64_t)p.items.size();  // [resources with requests]
    case B::sc_has: case B::sc_wants: case B::sc_sub:
      return std::max<int64_t>(p.scratch, 1);  // [rows of the requested resources]
    case B::res:
      return (int64_t)p.fitems.size();  // [fast items]
    case B::keys: case B::keys_s: case B::ps:
      return p.m;  // [sum n + 1]
    case B::ev_in: case B::evs_in: case B::ev: case B::evs:
      return p.e;  // [sum 2K]
    case B::ecnt: case B::esum:
      return p.b * (2 * kFdBlock + 1);  // [blocks * (2 kFdBlock + 1)]: a block's exclusive prefix, then its total
    case B::bdc: case B::bds:
      return p.b;  // [blocks]
    case B::pc: case B::pt:
      return p.c;  // [row chunks]
    case B::part:
      return p.parts;  // [scan chunks of the longest scan]
    case B::bounds:
      return 2 * p.b;  // [blocks] begins, [blocks] ends
  }
  return 0;
}

}  // namespace dm
