// The cases of tests/test_decide_plan.py: dm_decide_plan.h alone against a transcription of
// the host code dm_decide held before the header existed (written from that code, not from the
// header: the request checks, the grouping, the work items, the fast path's areas, the event
// blocks' bounds and the count each `ensure` or `upload` line gave its buffer; the upload of
// the FastItems is left out, no kernel read it).  Every field the two produce is compared,
// and the plan is checked against what the kernels index (independent of both).  Then one
// line per named case:
//   <case> <error> order=<first 8> items=<seg>:<fast>:<qlo>-<qhi>@<scr>,... scratch=<s>
//     fast=<item>:<k0>+<K>:n<n>:blk<nblk>:ch<nch>:<m0>/<e0>/<b0>/<c0>:r<repeats>,...
//     mebc=<m>/<e>/<b>/<c> parts=<p> last_end=<last end bound> prev=<links set>
#include <cstdio>
#include <string>

#include "dm_decide_plan.h"

using namespace dm;

constexpr int64_t kSubMaxT = 0x7FFFFFFE;

// ---- the parent's code, transcribed ----------------------------------------------------
namespace parent {
enum { DM_OK = 0, DM_E_RANGE = 1, DM_E_INVAL = 2 };  // any distinct codes
struct Ctx {  // what the function read of the context
  std::vector<int64_t> h_seg_off;
  int64_t N;
  bool decide_fast;
};
struct Out {
  int rc = DM_OK;
  std::vector<int64_t> order, srows, prev, bounds;
  std::vector<ReqItem> items;
  std::vector<FastItem> fitems;
  int64_t scratch = 0, m_off = 0, e_off = 0, b_off = 0, c_off = 0;
  int neb = 0;
  int64_t count[kRoundBufs] = {};  // 0: the buffer was not touched
};
inline Out decide(const Ctx* c, int64_t n, const int64_t* rows, const int64_t* subclients) {
  Out o;
  auto ensured = [&o](RoundBuf b, size_t count) { o.count[(int)b] = (int64_t)count; };
  std::vector<int64_t> seg_of((size_t)n);
  for (int64_t k = 0; k < n; ++k) {
    const int64_t r = rows[k];
    if (r < 0 || r >= c->N) return o.rc = DM_E_RANGE, o;
    if (subclients[k] < 0 || subclients[k] > kSubMaxT) return o.rc = DM_E_INVAL, o;
    seg_of[(size_t)k] = std::upper_bound(c->h_seg_off.begin(), c->h_seg_off.end(), r) - c->h_seg_off.begin() - 1;
  }
  std::vector<int64_t>& order = o.order;
  order.resize((size_t)n);
  for (int64_t i = 0; i < n; ++i) order[(size_t)i] = i;
  std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return seg_of[(size_t)a] < seg_of[(size_t)b]; });
  std::vector<int64_t>& srows = o.srows;
  srows.resize((size_t)n);
  std::vector<ReqItem>& items = o.items;
  int64_t scratch = 0;
  for (int64_t i = 0; i < n; ++i) {
    const int64_t k = order[(size_t)i], seg = seg_of[(size_t)k];
    srows[(size_t)i] = rows[k];
    if (items.empty() || items.back().seg != (int32_t)seg) {
      items.push_back(ReqItem{(int32_t)seg, 0, i, i, scratch});
      scratch += c->h_seg_off[seg + 1] - c->h_seg_off[seg];
    }
    items.back().qhi = i + 1;
  }
  std::vector<FastItem>& fitems = o.fitems;
  std::vector<int64_t>& prev = o.prev;
  int64_t m_off = 0, e_off = 0, b_off = 0, c_off = 0;
  for (size_t ii = 0; c->decide_fast && ii < items.size(); ++ii) {
    ReqItem& itm = items[ii];
    const int64_t K = itm.qhi - itm.qlo;
    if (K < kFdMin) continue;
    if (prev.empty()) prev.assign((size_t)n, -1);
    FastItem f{};
    f.item = (int32_t)ii;
    f.k0 = itm.qlo;
    f.K = K;
    f.n = c->h_seg_off[itm.seg + 1] - c->h_seg_off[itm.seg];
    f.nblk = (int32_t)((K + kFdBlock - 1) / kFdBlock);
    f.m0 = m_off;
    f.e0 = e_off;
    f.b0 = b_off;
    f.c0 = c_off;
    f.nch = (int32_t)std::max<int64_t>(1, (f.n + kFdRows - 1) / kFdRows);
    m_off += f.n + 1;
    e_off += 2 * K;
    b_off += f.nblk;
    c_off += f.nch;
    itm.fast = (int32_t)fitems.size() + 1;
    fitems.push_back(f);
    std::unordered_map<int64_t, int64_t> last;
    last.reserve((size_t)(2 * K));
    for (int64_t k = itm.qlo; k < itm.qhi; ++k) {
      auto f2 = last.find(srows[(size_t)k]);
      if (f2 != last.end()) {
        prev[(size_t)k] = f2->second;
        fitems.back().repeats = 1;
      }
      last[srows[(size_t)k]] = k;
    }
  }
  ensured(RoundBuf::rows, (size_t)n);  // upload(c->rq_rows, srows.data(), (size_t)n, st)
  ensured(RoundBuf::has, (size_t)n);
  ensured(RoundBuf::wants, (size_t)n);
  ensured(RoundBuf::sub, (size_t)n);
  ensured(RoundBuf::items, items.size());
  ensured(RoundBuf::gets, (size_t)n);
  ensured(RoundBuf::exp, (size_t)n);
  ensured(RoundBuf::sc_has, (size_t)std::max<int64_t>(scratch, 1));
  ensured(RoundBuf::sc_wants, (size_t)std::max<int64_t>(scratch, 1));
  ensured(RoundBuf::sc_sub, (size_t)std::max<int64_t>(scratch, 1));
  const int nfast = (int)fitems.size();
  if (nfast > 0) {
    ensured(RoundBuf::prev, prev.size());  // upload(c->fd_prev, prev.data(), prev.size(), st)
    ensured(RoundBuf::res, (size_t)nfast);
    ensured(RoundBuf::pw, (size_t)n);
    ensured(RoundBuf::v, (size_t)n);
    ensured(RoundBuf::sc, (size_t)n);
    ensured(RoundBuf::keys, (size_t)m_off);
    ensured(RoundBuf::keys_s, (size_t)m_off);
    ensured(RoundBuf::ps, (size_t)m_off);
    ensured(RoundBuf::ev_in, (size_t)e_off);
    ensured(RoundBuf::evs_in, (size_t)e_off);
    ensured(RoundBuf::ev, (size_t)e_off);
    ensured(RoundBuf::evs, (size_t)e_off);
    ensured(RoundBuf::ecnt, (size_t)(b_off * (2 * kFdBlock + 1)));
    ensured(RoundBuf::esum, (size_t)(b_off * (2 * kFdBlock + 1)));
    ensured(RoundBuf::bdc, (size_t)b_off);
    ensured(RoundBuf::bds, (size_t)b_off);
    ensured(RoundBuf::pc, (size_t)c_off);
    ensured(RoundBuf::pt, (size_t)c_off);
    ensured(RoundBuf::ld, (size_t)n);
    int64_t most = 1;
    for (const FastItem& f : fitems) most = std::max(most, std::max(f.K, f.n + 1));
    ensured(RoundBuf::part, (size_t)((most + kFdChunk - 1) / kFdChunk));
    // segment bounds of the event blocks' sort
    std::vector<int64_t> eb, ee;
    for (const FastItem& f : fitems)
      for (int64_t b = 0; b < f.nblk; ++b) {
        eb.push_back(f.e0 + 2 * b * kFdBlock);
        ee.push_back(f.e0 + 2 * std::min<int64_t>(f.K, (b + 1) * kFdBlock));
      }
    o.neb = (int)eb.size();
    std::vector<int64_t> bounds(eb);
    bounds.insert(bounds.end(), ee.begin(), ee.end());
    ensured(RoundBuf::bounds, bounds.size());  // d_eb = fd_bounds.p, d_ee = d_eb + eb.size()
    o.bounds = bounds;
  }
  o.scratch = scratch, o.m_off = m_off, o.e_off = e_off, o.b_off = b_off, o.c_off = c_off;
  return o;
}
}  // namespace parent

// ---- the cases -------------------------------------------------------------------------
struct Case {
  std::string name;
  std::vector<int64_t> sizes;  // rows per resource
  std::vector<int64_t> rows, sub;
  bool fast = true;
  bool shown = false;
  void ask(int64_t row, int64_t s = 1) { rows.push_back(row), sub.push_back(s); }
  int64_t base(int r) const {
    int64_t b = 0;
    for (int i = 0; i < r; ++i) b += sizes[(size_t)i];
    return b;
  }
  // K requests on resource r, on its rows from 0 up (wrapping: a resource smaller than K is asked again)
  void ask_many(int r, int64_t K) {
    for (int64_t k = 0; k < K; ++k) ask(base(r) + k % sizes[(size_t)r]);
  }
};

static std::vector<Case> cases() {
  std::vector<Case> cs;
  auto add = [&cs](const char* name, std::vector<int64_t> sizes, bool shown = false) -> Case& {
    cs.push_back(Case{name, std::move(sizes), {}, {}, true, shown});
    return cs.back();
  };
  // the fast-path threshold
  add("below_min", {100}, true).ask_many(0, kFdMin - 1);
  add("at_min", {100}, true).ask_many(0, kFdMin);
  {
    Case& c = add("small_between", {100, 100, 100}, true);
    for (int k = 0; k < kFdMin; ++k) c.ask(c.base(2) + k), c.ask(c.base(0) + k);
    for (int k = 0; k < kFdMin - 1; ++k) c.ask(c.base(1) + k);
  }
  // event-block and scan-chunk boundaries, on a resource smaller than K (rows asked again)
  // and on one with n + 1 > K; a second fast item behind shows the offsets that follow
  for (int64_t K : {(int64_t)kFdBlock, (int64_t)kFdBlock + 1, (int64_t)kFdChunk, (int64_t)kFdChunk + 1,
                    (int64_t)2 * kFdBlock, (int64_t)2 * kFdBlock + 1})
    for (int64_t n : {(int64_t)50, K - 1, K, K + 500}) {
      Case& c = add(("K" + std::to_string(K) + "_n" + std::to_string(n)).c_str(), {n, 80}, n == K + 500 && K <= kFdBlock + 1);
      c.ask_many(0, K);
      c.ask_many(1, kFdMin);
    }
  // row-chunk boundaries
  for (int64_t n : {(int64_t)1, (int64_t)kFdRows, (int64_t)kFdRows + 1, (int64_t)2 * kFdRows, (int64_t)2 * kFdRows + 1}) {
    Case& c = add(("rows" + std::to_string(n)).c_str(), {n, 70}, n <= kFdRows + 1);
    c.ask_many(0, kFdMin);
    c.ask_many(1, kFdMin + 1);
  }
  // repeats
  {
    Case& c = add("one_row_chain", {9, 100}, true);
    c.ask(0);  // another resource before it: the links are grouped indices, not the resource's own
    for (int k = 0; k < 70; ++k) c.ask(c.base(1) + 5);
  }
  {
    Case& c = add("one_row_twice", {100, 100}, true);
    for (int k = 0; k < 70; ++k) c.ask(c.base(1) + k), c.ask(k);  // the same local rows on two resources
    c.ask(c.base(1) + 7);
  }
  add("no_repeats", {100}).ask_many(0, 100);
  // stable grouping: three resources' requests interleaved, rows descending within each
  {
    Case& c = add("interleaved", {4, 5, 6}, true);
    for (int k = 0; k < 4; ++k) c.ask(c.base(2) + 5 - k), c.ask(c.base(0) + 3 - k), c.ask(c.base(1) + 4 - k);
  }
  for (bool fast : {true, false}) {
    Case& c = add(fast ? "interleaved_fast" : "interleaved_fast_off", {90, 5, 200}, !fast);
    c.fast = fast;
    for (int k = 0; k < 130; ++k) {
      c.ask(c.base(2) + (k * 7) % 200), c.ask(c.base(0) + (k * 5) % 90);
      if (k % 40 == 0) c.ask(c.base(1) + 4 - k / 40);
    }
  }
  // resources of differing sizes: the scratch offsets (resources without requests take none)
  {
    Case& c = add("scratch_offsets", {5, 300, 1, 4097, 12}, true);
    c.ask(c.base(3) + 4096), c.ask(c.base(0)), c.ask(c.base(2)), c.ask(c.base(4) + 11), c.ask(c.base(0) + 4);
  }
  // row 0 and row N - 1
  {
    Case& c = add("extreme_rows", {3, 2, 70}, true);
    c.ask(c.base(2) + 69), c.ask(0);
    for (int k = 0; k < 64; ++k) c.ask(c.base(2) + 69 - k);
  }
  // the four rejections, each behind a valid request; then the order of two failures
  add("row_minus_1", {10}, true).ask(3);
  cs.back().ask(-1);
  add("row_N", {10}, true).ask(9);
  cs.back().ask(10);
  add("sub_minus_1", {10}, true).ask(3);
  cs.back().ask(4, -1);
  add("sub_over_max", {10}, true).ask(3, kSubMaxT);
  cs.back().ask(4, kSubMaxT + 1);
  {
    Case& c = add("sub_fails_before_row", {10}, true);
    c.ask(1), c.ask(2, -1), c.ask(10);
  }
  {
    Case& c = add("row_fails_before_sub", {10}, true);
    c.ask(1), c.ask(10), c.ask(2, -1);
  }
  add("one_request_fails_both", {10}, true).ask(1);
  cs.back().ask(-1, -1);
  // mixed rounds: a deterministic sweep of sizes and request counts around every threshold
  uint64_t s = 12345;
  auto rnd = [&s](uint64_t m) { return (s = s * 6364136223846793005ull + 1442695040888963407ull, (s >> 33) % m); };
  const int64_t edge_n[] = {1, 2, 63, 64, 65, 1023, 1024, 2047, 2048, 4095, 4096, 4097, 8193};
  const int64_t edge_k[] = {0, 1, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 4097};
  for (int i = 0; i < 150; ++i) {
    Case& c = add(("mixed" + std::to_string(i)).c_str(), {});
    const int R = 1 + (int)rnd(5);
    for (int r = 0; r < R; ++r) c.sizes.push_back(edge_n[rnd(13)]);
    std::vector<int64_t> left;
    for (int r = 0; r < R; ++r) left.push_back(edge_k[rnd(12)]);
    c.fast = rnd(8) != 0;
    for (bool any = true; any;) {  // the resources' requests interleaved at random, rows at random
      any = false;
      for (int r = 0; r < R; ++r) {
        const int64_t take = std::min<int64_t>(left[(size_t)r], 1 + (int64_t)rnd(3));
        for (int64_t k = 0; k < take; ++k) c.ask(c.base(r) + (int64_t)rnd((uint64_t)c.sizes[(size_t)r]), 1 + (int64_t)rnd(3));
        left[(size_t)r] -= take;
        any = any || left[(size_t)r] > 0;
      }
    }
    if (c.rows.empty()) c.ask(0);
  }
  return cs;
}

// ---- comparison ------------------------------------------------------------------------
static int64_t differ = 0;
template <typename A, typename B>
static void same(const A& a, const B& b) {
  differ += !((int64_t)a == (int64_t)b);
}
static void same_vec(const std::vector<int64_t>& a, const std::vector<int64_t>& b) {
  differ += a.size() != b.size();
  for (size_t i = 0; i < std::min(a.size(), b.size()); ++i) same(a[i], b[i]);
}

static void compare(const RoundPlan& p, const parent::Out& o) {
  same((int)p.error, o.rc == parent::DM_OK ? 0 : o.rc == parent::DM_E_RANGE ? 1 : 2);
  same_vec(p.order, o.order);
  same(p.items.size(), o.items.size());
  for (size_t i = 0; i < std::min(p.items.size(), o.items.size()); ++i) {
    const ReqItem &a = p.items[i], &b = o.items[i];
    same(a.seg, b.seg), same(a.fast, b.fast), same(a.qlo, b.qlo), same(a.qhi, b.qhi), same(a.scr, b.scr);
  }
  same(p.scratch, o.scratch);
  same(p.fitems.size(), o.fitems.size());
  for (size_t i = 0; i < std::min(p.fitems.size(), o.fitems.size()); ++i) {
    const FastItem &a = p.fitems[i], &b = o.fitems[i];
    same(a.item, b.item), same(a.nblk, b.nblk), same(a.k0, b.k0), same(a.K, b.K), same(a.m0, b.m0), same(a.e0, b.e0);
    same(a.b0, b.b0), same(a.n, b.n), same(a.c0, b.c0), same(a.nch, b.nch), same(a.repeats, b.repeats);
  }
  same_vec(p.prev, o.prev);
  same(p.m, o.m_off), same(p.e, o.e_off), same(p.b, o.b_off), same(p.c, o.c_off);
  same(p.b, o.neb);  // the pair sort's segments
  same_vec(p.bounds, o.bounds);
  if (p.error == RoundError::none)
    for (int b = 0; b < kRoundBufs; ++b) same(round_count(p, (RoundBuf)b), o.count[b]);
}

// What the kernels of dm_decide_fast.hip and dm_round.hip index, against the plan's counts.
static int64_t broken = 0;
static void holds(bool ok) { broken += !ok; }
static void invariants(const Case& c, const RoundPlan& p) {
  if (p.error != RoundError::none) return;
  auto cnt = [&p](RoundBuf b) { return round_count(p, b); };
  const int64_t n = (int64_t)c.rows.size();
  std::vector<int> seen((size_t)n, 0);
  for (int64_t i : p.order) holds(i >= 0 && i < n && !seen[(size_t)i]++);
  int64_t q = 0, scr = 0;
  for (const ReqItem& it : p.items) {
    const int64_t rows_of = c.sizes[(size_t)it.seg];
    holds(it.qlo == q && it.qhi > it.qlo && it.scr == scr);
    for (int64_t k = it.qlo; k < it.qhi; ++k) {
      const int64_t row = c.rows[(size_t)p.order[(size_t)k]];
      holds(row >= c.base(it.seg) && row < c.base(it.seg) + rows_of);
      holds(k == it.qlo || p.order[(size_t)k - 1] < p.order[(size_t)k]);  // stable
    }
    q = it.qhi, scr += rows_of;
    holds(it.fast == 0 || (c.fast && it.qhi - it.qlo >= kFdMin));
    holds(it.fast != 0 || !c.fast || it.qhi - it.qlo < kFdMin);
  }
  holds(q == n && scr == p.scratch && scr <= cnt(RoundBuf::sc_has) && scr <= cnt(RoundBuf::sc_sub));
  holds(p.prev.empty() == p.fitems.empty());
  int64_t m = 0, e = 0, b = 0, ch = 0;
  for (size_t s = 0; s < p.fitems.size(); ++s) {
    const FastItem& f = p.fitems[s];
    const ReqItem& it = p.items[(size_t)f.item];
    holds(it.fast == (int32_t)s + 1 && f.k0 == it.qlo && f.K == it.qhi - it.qlo && f.n == c.sizes[(size_t)it.seg]);
    holds(f.m0 == m && f.e0 == e && f.b0 == b && f.c0 == ch);  // the areas are disjoint and dense
    holds((int64_t)f.nblk * kFdBlock >= f.K && ((int64_t)f.nblk - 1) * kFdBlock < f.K);
    holds((int64_t)f.nch * kFdRows >= f.n && f.nch >= 1);
    m += f.n + 1, e += 2 * f.K, b += f.nblk, ch += f.nch;
    holds(m <= cnt(RoundBuf::keys) && m <= cnt(RoundBuf::ps) && e <= cnt(RoundBuf::ev) && e <= cnt(RoundBuf::evs_in));
    holds(b * (2 * kFdBlock + 1) <= cnt(RoundBuf::ecnt) && b <= cnt(RoundBuf::bds) && ch <= cnt(RoundBuf::pc));
    holds((std::max(f.K, f.n + 1) + kFdChunk - 1) / kFdChunk <= cnt(RoundBuf::part));
    holds(f.k0 + f.K <= cnt(RoundBuf::ld) && (int64_t)s < cnt(RoundBuf::res));
    // a request's link: the nearest earlier request of the resource on the same row
    std::vector<std::pair<int64_t, int64_t>> by_row;  // (row, grouped index), sorted
    for (int64_t k = f.k0; k < f.k0 + f.K; ++k) by_row.push_back({c.rows[(size_t)p.order[(size_t)k]], k});
    std::sort(by_row.begin(), by_row.end());
    int rep = 0;
    for (size_t j = 0; j < by_row.size(); ++j) {
      const bool again = j > 0 && by_row[j - 1].first == by_row[j].first;
      holds(p.prev[(size_t)by_row[j].second] == (again ? by_row[j - 1].second : -1));
      rep |= again;
    }
    holds(f.repeats == rep);
    for (int64_t j = 0; j < f.nblk; ++j) {  // the blocks tile the item's events
      const int64_t lo = p.bounds[(size_t)(f.b0 + j)], hi = p.bounds[(size_t)(p.b + f.b0 + j)];
      holds(lo == f.e0 + 2 * j * kFdBlock && hi > lo && hi - lo <= 2 * kFdBlock);
      holds(j + 1 < f.nblk ? hi == p.bounds[(size_t)(f.b0 + j + 1)] : hi == f.e0 + 2 * f.K);
    }
  }
  holds(m == p.m && e == p.e && b == p.b && ch == p.c && (int64_t)p.bounds.size() == cnt(RoundBuf::bounds));
  for (size_t k = 0; k < p.prev.size(); ++k)  // requests outside the fast items keep no link
    if (p.prev[k] >= 0) {
      bool inside = false;
      for (const FastItem& f : p.fitems) inside = inside || ((int64_t)k >= f.k0 && (int64_t)k < f.k0 + f.K);
      holds(inside);
    }
}

static void show(const Case& c, const RoundPlan& p) {
  const char* err[] = {"ok", "row_range", "subclients"};
  std::printf("%s %s", c.name.c_str(), err[(int)p.error]);
  if (p.error != RoundError::none) {
    std::printf("\n");
    return;
  }
  std::printf(" order=");
  for (size_t i = 0; i < std::min<size_t>(p.order.size(), 8); ++i) std::printf("%s%lld", i ? "," : "", (long long)p.order[i]);
  std::printf(" items=");
  for (size_t i = 0; i < p.items.size(); ++i)
    std::printf("%s%d:%d:%lld-%lld@%lld", i ? "," : "", p.items[i].seg, p.items[i].fast, (long long)p.items[i].qlo,
                (long long)p.items[i].qhi, (long long)p.items[i].scr);
  std::printf(" scratch=%lld fast=", (long long)p.scratch);
  for (size_t i = 0; i < p.fitems.size(); ++i) {
    const FastItem& f = p.fitems[i];
    std::printf("%s%d:%lld+%lld:n%lld:blk%d:ch%d:%lld/%lld/%lld/%lld:r%d", i ? "," : "", f.item, (long long)f.k0, (long long)f.K,
                (long long)f.n, f.nblk, f.nch, (long long)f.m0, (long long)f.e0, (long long)f.b0, (long long)f.c0, f.repeats);
  }
  int64_t links = 0;
  for (int64_t v : p.prev) links += v >= 0;
  std::printf("%s mebc=%lld/%lld/%lld/%lld parts=%lld last_end=%lld prev=%s%lld\n", p.fitems.empty() ? "-" : "", (long long)p.m,
              (long long)p.e, (long long)p.b, (long long)p.c, (long long)p.parts, (long long)(p.bounds.empty() ? -1 : p.bounds.back()),
              p.prev.empty() ? "empty:" : "", (long long)links);
}

int main() {
  const std::vector<Case> cs = cases();
  std::vector<RoundPlan> plans;
  int64_t fast_rounds = 0, rejected = 0;
  for (const Case& c : cs) {
    parent::Ctx ctx{{0}, 0, c.fast};
    for (int64_t sz : c.sizes) ctx.h_seg_off.push_back(ctx.h_seg_off.back() + sz);
    ctx.N = ctx.h_seg_off.back();
    const int64_t n = (int64_t)c.rows.size();
    const parent::Out o = parent::decide(&ctx, n, c.rows.data(), c.sub.data());
    plans.push_back(plan_round(ctx.h_seg_off.data(), (int64_t)c.sizes.size(), ctx.N, c.rows.data(), c.sub.data(), n, c.fast,
                               kSubMaxT));
    compare(plans.back(), o);
    invariants(c, plans.back());
    fast_rounds += plans.back().fast();
    rejected += plans.back().error != RoundError::none;
  }
  std::printf("cases %zu disagreements %lld invariant_violations %lld (fast rounds %lld rejected %lld)\n", cs.size(),
              (long long)differ, (long long)broken, (long long)fast_rounds, (long long)rejected);
  for (size_t i = 0; i < cs.size(); ++i)
    if (cs[i].shown) show(cs[i], plans[i]);
  return 0;
}
