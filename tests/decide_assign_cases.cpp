// The cases of tests/test_decide_assign_plan.py: dm_decide_assign.h's assign_selection alone,
// over plan_round's plan (dm_decide_plan.h), against a plain restatement with a map: for every
// distinct row the caller's last request on it, found in the caller's order, then looked up
// in the plan's grouped order.  Per round: exactly one position per distinct row, that
// position the row's last request, ascending order, every position inside the round, and
// counts that cover what the gather kernel (dm_decide_assign.hip) indexes.  One line per case:
//   <case> n=<requests> m=<selected> sel=<first 8 positions> rows=<their rows> breaches=<count>
// and a first line with the totals.
#include <cstdio>
#include <map>
#include <string>

#include "dm_decide_assign.h"

using namespace dm;

struct Round {
  std::string name;
  std::vector<int64_t> seg_off;
  std::vector<int64_t> rows;
};

static int check(const Round& rd, std::string* line) {
  const int64_t R = (int64_t)rd.seg_off.size() - 1, N = rd.seg_off.back(), n = (int64_t)rd.rows.size();
  const std::vector<int64_t> sub((size_t)n, 1);
  const RoundPlan plan = plan_round(rd.seg_off.data(), R, N, rd.rows.data(), sub.data(), n, true, 0x7FFFFFFE);
  int bad = plan.error != RoundError::none;
  const AssignSel a = assign_selection(plan, rd.rows.data());
  // the restatement: the caller's last request on each row ...
  std::map<int64_t, int64_t> last;
  for (int64_t k = 0; k < n; ++k) last[rd.rows[(size_t)k]] = k;
  // ... and where the grouped order put each of the caller's requests
  std::vector<int64_t> pos((size_t)n, -1);
  for (int64_t i = 0; i < n; ++i) pos[(size_t)plan.order[(size_t)i]] = i;
  std::map<int64_t, int64_t> want;  // grouped position -> row
  for (const auto& kv : last) want[pos[(size_t)kv.second]] = kv.first;
  bad += a.n != n;
  bad += a.m() != (int64_t)last.size();  // one position per distinct row
  std::map<int64_t, int> seen;
  for (int64_t j = 0; j < a.m(); ++j) {
    const int64_t i = a.sel[(size_t)j];
    if (i < 0 || i >= n) {  // what k_assign_gather indexes the grouped columns with
      ++bad;
      continue;
    }
    const int64_t row = rd.rows[(size_t)plan.order[(size_t)i]];
    bad += ++seen[row] != 1;                                  // exactly one
    bad += plan.order[(size_t)i] != last[row];                // the row's last request
    bad += j > 0 && a.sel[(size_t)(j - 1)] >= i;              // ascending
    bad += !want.count(i) || want[i] != row;                  // the restatement's position
  }
  // counts: the selection and the five compact columns hold m entries (lane j < m writes entry
  // j), the safe capacities one per request (lane k < n writes entry k)
  for (AssignBuf b : {AssignBuf::sel, AssignBuf::rows, AssignBuf::has, AssignBuf::wants, AssignBuf::sub, AssignBuf::exp})
    bad += assign_count(a, b) != a.m() || assign_count(a, b) < 1;
  bad += assign_count(a, AssignBuf::safe) != n;
  char buf[64];
  snprintf(buf, sizeof buf, " n=%lld m=%lld sel=", (long long)n, (long long)a.m());
  *line = rd.name + buf;
  for (int64_t j = 0; j < a.m() && j < 8; ++j) *line += (j ? "," : "") + std::to_string(a.sel[(size_t)j]);
  *line += " rows=";
  for (int64_t j = 0; j < a.m() && j < 8; ++j) {
    const int64_t i = a.sel[(size_t)j];
    *line += (j ? "," : "") + (i >= 0 && i < n ? std::to_string(rd.rows[(size_t)plan.order[(size_t)i]]) : "?");
  }
  *line += " breaches=" + std::to_string(bad);
  return bad;
}

int main() {
  // three resources of 10, 100 and 20 rows: rows 0-9, 10-109, 110-129
  const std::vector<int64_t> off = {0, 10, 110, 130};
  std::vector<Round> rounds;
  rounds.push_back({"no_repeats", off, {3, 12, 111, 4, 13}});
  rounds.push_back({"twice_adjacent", off, {3, 3, 12}});
  rounds.push_back({"thrice_adjacent", off, {12, 12, 12, 3}});
  rounds.push_back({"twice_interleaved", off, {12, 3, 111, 12, 4}});  // other rows and other resources between
  rounds.push_back({"thrice_interleaved", off, {12, 111, 13, 12, 3, 14, 12, 112}});
  rounds.push_back({"two_rows_interleaved", off, {12, 13, 12, 13, 111, 13}});
  rounds.push_back({"all_on_one_row", off, std::vector<int64_t>(9, 57)});
  rounds.push_back({"one_request", off, {129}});
  {
    Round r{"k64_one_resource", off, {}};  // the fast path's threshold (kFdMin): 64 requests ...
    for (int k = 0; k < 64; ++k) r.rows.push_back(10 + k);
    r.rows[63] = 10;  // ... the last of them a repeat of the first
    rounds.push_back(r);
    Round s{"k65_one_resource", off, {}};  // ... and 65, beside requests on another resource
    for (int k = 0; k < 65; ++k) s.rows.push_back(10 + k % 50);
    s.rows.push_back(2);
    s.rows.insert(s.rows.begin(), 2);
    rounds.push_back(s);
  }
  rounds.push_back({"descending_resources", off, {120, 111, 120, 50, 10, 50, 9, 0, 9}});
  // a fixed sweep of mixed rounds: every length up to 40 over few rows, so repeats are common
  uint64_t x = 88172645463325252ull;
  auto rnd = [&x] {
    x ^= x << 13, x ^= x >> 7, x ^= x << 17;
    return x;
  };
  for (int n = 1; n <= 40; ++n) {
    Round r{"sweep" + std::to_string(n), off, {}};
    for (int k = 0; k < n; ++k) r.rows.push_back((int64_t)(rnd() % (n % 3 ? 130 : 12)));
    rounds.push_back(r);
  }
  int total = 0, named = 0;
  std::vector<std::string> lines;
  for (const Round& r : rounds) {
    std::string line;
    total += check(r, &line);
    if (r.name.compare(0, 5, "sweep") != 0) lines.push_back(line), ++named;
  }
  printf("cases %d named %d breaches %d\n", (int)rounds.size(), named, total);
  for (const std::string& l : lines) printf("%s\n", l.c_str());
  return 0;
}
