// propose_plan_driver.cpp — stand-alone check of raft_propose's host plan
// (raft-sample_amd/csrc/propose_plan.hpp), built with the host compiler under
// -fsanitize=address,undefined and run as a child process by
// tests/test_propose_model.py. Nothing of it is loaded into Python.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../raft-sample_amd/csrc/propose_plan.hpp"

using raftstep::ProposePlan;

namespace {

struct Prop {   // raft_proposal's layout
  uint64_t group;
  int64_t value;
};

int failures = 0;
#define CHECK(c)                                                         \
  do {                                                                   \
    if (!(c)) {                                                          \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);              \
      ++failures;                                                        \
    }                                                                    \
  } while (0)

// The plan against its definition: perm is a permutation, sorted by group,
// list order kept inside a group (stability), and the segment starts are
// exactly the places where the group changes.
void check_plan(const std::vector<Prop>& p, uint64_t G, const char* what) {
  ProposePlan plan;
  uint64_t bad = ~uint64_t(0);
  const int rc = raftstep::propose_plan(p.data(), sizeof(Prop), p.size(), G, &plan, &bad);
  CHECK(rc == raftstep::PLAN_OK);
  const size_t n = p.size();
  CHECK(plan.perm.size() == n);
  CHECK(plan.seg.size() >= 1 && plan.seg.front() == 0 && plan.seg.back() == n);
  if (failures) {
    printf("  in case %s\n", what);
    return;
  }
  std::vector<char> seen(n, 0);
  for (size_t i = 0; i < n; ++i) {
    CHECK(plan.perm[i] < n && !seen[plan.perm[i]]);
    seen[plan.perm[i]] = 1;
    if (i) {
      const Prop &a = p[plan.perm[i - 1]], &b = p[plan.perm[i]];
      CHECK(a.group < b.group || (a.group == b.group && plan.perm[i - 1] < plan.perm[i]));
    }
  }
  std::vector<uint32_t> want;
  for (size_t i = 0; i < n; ++i)
    if (!i || p[plan.perm[i]].group != p[plan.perm[i - 1]].group) want.push_back(uint32_t(i));
  want.push_back(uint32_t(n));
  CHECK(want == plan.seg);
  CHECK(plan.segments() + 1 == plan.seg.size());
  if (failures) printf("  in case %s\n", what);
}

}  // namespace

int main() {
  const uint64_t G = 577;
  {   // the empty list
    ProposePlan plan;
    CHECK(raftstep::propose_plan(nullptr, sizeof(Prop), 0, G, &plan, nullptr) == raftstep::PLAN_OK);
    CHECK(plan.perm.empty() && plan.seg.size() == 1 && plan.seg[0] == 0 && plan.segments() == 0);
  }
  check_plan({{42, 7}}, G, "n = 1");
  {   // one hot group
    std::vector<Prop> p(5000);
    for (size_t i = 0; i < p.size(); ++i) p[i] = {123, int64_t(i)};
    check_plan(p, G, "one group, n = 5000");
    ProposePlan plan;
    raftstep::propose_plan(p.data(), sizeof(Prop), p.size(), G, &plan, nullptr);
    CHECK(plan.segments() == 1);
    for (size_t i = 0; i < p.size(); ++i) CHECK(plan.perm[i] == i);
  }
  {   // all distinct: ascending, descending, shuffled
    std::vector<Prop> a(G), d(G), s(G);
    for (uint64_t i = 0; i < G; ++i) {
      a[i] = {i, int64_t(i)};
      d[i] = {G - 1 - i, int64_t(i)};
      s[i] = {(i * 211) % G, int64_t(i)};   // (211 and 577 are coprime)
    }
    check_plan(a, G, "distinct ascending");
    check_plan(d, G, "distinct descending");
    check_plan(s, G, "distinct shuffled");
    ProposePlan plan;
    raftstep::propose_plan(d.data(), sizeof(Prop), G, G, &plan, nullptr);
    CHECK(plan.segments() == G && plan.perm[0] == G - 1);
  }
  {   // interleaved repeats: 3, 1, 3, 2, 1, 3, ...
    std::vector<Prop> p;
    const uint64_t ids[] = {3, 1, 3, 2, 1, 3, 576, 0, 3, 576};
    for (int rep = 0; rep < 40; ++rep)
      for (uint64_t g : ids) p.push_back({g, int64_t(p.size())});
    check_plan(p, G, "interleaved repeats");
    ProposePlan plan;
    raftstep::propose_plan(p.data(), sizeof(Prop), p.size(), G, &plan, nullptr);
    CHECK(plan.segments() == 5);
    CHECK(plan.perm[0] == 7 && plan.perm[1] == 17);   // group 0: list positions 7, 17, ...
  }
  {   // range errors: the first bad position, nothing planned
    std::vector<Prop> p = {{1, 0}, {2, 0}, {G, 0}, {1ull << 63, 0}};
    ProposePlan plan;
    uint64_t bad = 99;
    CHECK(raftstep::propose_plan(p.data(), sizeof(Prop), p.size(), G, &plan, &bad) == raftstep::PLAN_RANGE && bad == 2);
    p[2].group = G - 1;
    CHECK(raftstep::propose_plan(p.data(), sizeof(Prop), p.size(), G, &plan, &bad) == raftstep::PLAN_RANGE && bad == 3);
    CHECK(raftstep::propose_plan(p.data(), sizeof(Prop), p.size(), G, &plan, nullptr) == raftstep::PLAN_RANGE);
    p[3].group = 0;
    check_plan(p, G, "after the repair");
    // a list longer than 2^31 is refused before any element is read
    CHECK(raftstep::propose_plan(p.data(), sizeof(Prop), (1ull << 31) + 1, G, &plan, &bad) == raftstep::PLAN_TOO_LONG);
    // the largest engine: ids up to 2^32 - 1 keep their order in the keys
    std::vector<Prop> q = {{0xFFFFFFFFull, 0}, {0, 1}, {0xFFFFFFFFull, 2}, {0x80000000ull, 3}};
    check_plan(q, 1ull << 32, "G = 2^32");
  }
  if (failures) {
    printf("propose plan driver: %d failures\n", failures);
    return 1;
  }
  printf("propose plan driver: ok\n");
  return 0;
}
