// Stand-alone driver of csrc/groups_host.cpp for the -fsanitize=address,undefined
// host build (tests/test_group_asan_host.py): cbv2_groups_build_host over random
// groupings with output arrays of EXACTLY the documented sizes (order [n],
// offsets [G + 1], labels [G], out3 [3]), so a write past any of them is a heap
// overflow the sanitizer reports, and every result checked against a plain
// recomputation.
#include <cstdint>
#include <cstdio>
#include <random>
#include <string>
#include <vector>

#include "colbert_mi355x.h"

static std::string g_last;
extern "C" int cbv2_set_error(int code, const char* msg) {
  g_last = msg ? msg : "";
  return code;
}

static int failed = 0;
#define CHECK(cond)                                             \
  do {                                                          \
    if (!(cond)) {                                              \
      ++failed;                                                 \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
    }                                                           \
  } while (0)

static void one_case(std::mt19937& rng, int64_t n, int32_t G, double none, int32_t used) {
  std::vector<int32_t> group_of((size_t)n);
  std::uniform_real_distribution<double> u(0.0, 1.0);
  for (auto& g : group_of) g = u(rng) < none ? -1 : (int32_t)(rng() % (uint32_t)used);
  // exact-size heap blocks: new[] of the documented extents
  int32_t* order = new int32_t[(size_t)n ? (size_t)n : 1];
  int32_t* offsets = new int32_t[(size_t)G + 1];
  int32_t* labels = new int32_t[(size_t)G];
  int64_t* out3 = new int64_t[3];
  const int rc = cbv2_groups_build_host(group_of.data(), n, G, order, offsets, labels, out3);
  CHECK(rc == CBV2_OK);
  if (rc == CBV2_OK) {
    std::vector<std::vector<int32_t>> want((size_t)G);
    int64_t members = 0, largest = 0;
    for (int64_t i = 0; i < n; ++i)
      if (group_of[(size_t)i] >= 0) want[(size_t)group_of[(size_t)i]].push_back((int32_t)i), ++members;
    int64_t s = 0, at = 0;
    for (int32_t g = 0; g < G; ++g) {
      if (want[(size_t)g].empty()) continue;
      CHECK(labels[s] == g && offsets[s] == at);
      for (size_t j = 0; j < want[(size_t)g].size(); ++j) CHECK(order[at + (int64_t)j] == want[(size_t)g][j]);
      at += (int64_t)want[(size_t)g].size();
      if ((int64_t)want[(size_t)g].size() > largest) largest = (int64_t)want[(size_t)g].size();
      ++s;
    }
    CHECK(offsets[s] == at && at == members);
    CHECK(out3[0] == members && out3[1] == s && out3[2] == largest);
  }
  // a value outside [-1, G): refused, the first offending position named, nothing written
  if (n > 0) {
    const int64_t at = (int64_t)(rng() % (uint64_t)n);
    const int32_t keep = group_of[(size_t)at];
    group_of[(size_t)at] = (rng() & 1) ? G : -2;
    for (int64_t i = 0; i < at; ++i)
      if (group_of[(size_t)i] < -1 || group_of[(size_t)i] >= G) group_of[(size_t)i] = -1;
    out3[0] = out3[1] = out3[2] = -99;
    offsets[0] = -99;
    CHECK(cbv2_groups_build_host(group_of.data(), n, G, order, offsets, labels, out3) == CBV2_EINVAL);
    CHECK(g_last.find("[" + std::to_string(at) + "]") != std::string::npos);
    CHECK(out3[0] == -99 && out3[1] == -99 && out3[2] == -99 && offsets[0] == -99);
    group_of[(size_t)at] = keep;
  }
  delete[] order;
  delete[] offsets;
  delete[] labels;
  delete[] out3;
}

int main() {
  std::mt19937 rng(2024);
  for (int64_t n : {0, 1, 31, 64, 65, 2049, 20011})
    for (int32_t G : {1, 2, 7, 1000})
      for (double none : {0.0, 0.3, 1.0}) {
        one_case(rng, n, G, none, G);                      // every group may have members
        one_case(rng, n, G, none, G > 3 ? G - 3 : 1);      // memberless groups at the end
      }
  int32_t dummy = 0;
  int64_t out3[3];
  CHECK(cbv2_groups_build_host(&dummy, 1, 0, &dummy, &dummy, &dummy, out3) == CBV2_EINVAL);
  CHECK(cbv2_groups_build_host(&dummy, -1, 1, &dummy, &dummy, &dummy, out3) == CBV2_EINVAL);
  CHECK(cbv2_groups_build_host(&dummy, (int64_t)1 << 31, 1, &dummy, &dummy, &dummy, out3) == CBV2_EINVAL);
  CHECK(cbv2_groups_build_host(nullptr, 1, 1, &dummy, &dummy, &dummy, out3) == CBV2_EINVAL);
  printf("%d failed checks\n", failed);
  return failed ? 1 : 0;
}
