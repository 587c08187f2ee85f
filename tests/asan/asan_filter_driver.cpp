// AddressSanitizer / UBSan driver for the filtered host BM25
// (cbv2_bm25_search_filtered): corpora whose last bitmap word is partial
// (n = 1, 31, 33, 257), empty and full filters and random ones, k above the
// allowed count, checked against a brute-force restatement (score every doc in
// posting order, drop the disallowed ones, sort by score desc / id asc, pad
// with -1).  The bitmaps are allocated with exactly ceil(n / 32) words, so a
// read past the last word is an ASan report.  Built by
// tests/test_asan_filter_host.py with g++ -fsanitize=address,undefined; test
// infrastructure only (no GPU code, no Python).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "colbert_mi355x.h"

extern "C" int cbv2_set_error(int code, const char* msg) {
  (void)msg;
  return code;
}

static int fails = 0;
#define CHECK(c)                                                           \
  do {                                                                     \
    if (!(c)) {                                                            \
      fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++fails;                                                             \
    }                                                                      \
  } while (0)

static void one_case(std::mt19937& rng, int N, int mode) {
  const int V = 1 + rng() % 20;
  std::vector<int64_t> off(N + 1, 0);
  std::vector<int32_t> terms;
  for (int d = 0; d < N; ++d) {
    const int len = rng() % 12;
    for (int t = 0; t < len; ++t) terms.push_back(rng() % V);
    off[d + 1] = (int64_t)terms.size();
  }
  cbv2_bm25* ix = nullptr;
  CHECK(cbv2_bm25_build(terms.empty() ? nullptr : terms.data(), off.data(), N, V, 1.5f, 0.75f, &ix) == CBV2_OK);
  if (!ix) return;
  // exactly ceil(N / 32) words on the heap; garbage past N in the last word
  const int nw = (N + 31) / 32;
  std::vector<uint32_t> allow(nw, 0u);
  std::vector<char> ok(N, 0);
  for (int d = 0; d < N; ++d) {
    ok[d] = mode == 0 ? 0 : mode == 1 ? 1 : (char)(rng() % 3 == 0);
    if (ok[d]) allow[d >> 5] |= 1u << (d & 31);
  }
  if (N & 31) allow[nw - 1] |= ~0u << (N & 31);
  int m = 0;
  for (int d = 0; d < N; ++d) m += ok[d];
  const int B = 4;
  std::vector<int64_t> qo(B + 1, 0);
  std::vector<int32_t> qt;
  for (int b = 0; b < B; ++b) {
    const int ql = b == 0 ? 0 : 1 + rng() % 5;
    for (int j = 0; j < ql; ++j) qt.push_back((int32_t)(rng() % (V + 2)) - 1);   // out-of-range ids too
    qo[b + 1] = (int64_t)qt.size();
  }
  // unfiltered scores of every doc: a search with k = N returns them all
  std::vector<int32_t> all_i((size_t)B * N);
  std::vector<float> all_s((size_t)B * N);
  CHECK(cbv2_bm25_search(ix, qt.empty() ? nullptr : qt.data(), qo.data(), B, N, 1, all_i.data(), all_s.data()) ==
        CBV2_OK);
  const int ks[3] = {1, m > 1 ? m - 1 : 1, m + 5};
  for (int k : ks) {
    std::vector<int32_t> ids((size_t)B * k, -7);
    std::vector<float> sc((size_t)B * k, -7.0f);
    CHECK(cbv2_bm25_search_filtered(ix, qt.empty() ? nullptr : qt.data(), qo.data(), B, k, 1 + k % 3, allow.data(),
                                    ids.data(), sc.data()) == CBV2_OK);
    for (int b = 0; b < B; ++b) {
      int j = 0;
      for (int r = 0; r < N && j < k; ++r) {   // the full ranking with the disallowed docs dropped
        const int32_t d = all_i[(size_t)b * N + r];
        if (d < 0 || !ok[d]) continue;
        CHECK(ids[(size_t)b * k + j] == d);
        CHECK(sc[(size_t)b * k + j] == all_s[(size_t)b * N + r]);
        ++j;
      }
      CHECK(j == std::min(k, m));
      for (; j < k; ++j) CHECK(ids[(size_t)b * k + j] == -1 && sc[(size_t)b * k + j] == 0.0f);
    }
    // scores are optional
    CHECK(cbv2_bm25_search_filtered(ix, qt.empty() ? nullptr : qt.data(), qo.data(), B, k, 2, allow.data(), ids.data(),
                                    nullptr) == CBV2_OK);
  }
  // allow == NULL is the unfiltered search
  std::vector<int32_t> a((size_t)B * 9), c((size_t)B * 9);
  CHECK(cbv2_bm25_search(ix, qt.empty() ? nullptr : qt.data(), qo.data(), B, 9, 1, a.data(), nullptr) == CBV2_OK);
  CHECK(cbv2_bm25_search_filtered(ix, qt.empty() ? nullptr : qt.data(), qo.data(), B, 9, 1, nullptr, c.data(),
                                  nullptr) == CBV2_OK);
  CHECK(a == c);
  cbv2_bm25_destroy(ix);
}

int main() {
  std::mt19937 rng(12345);
  const int ns[4] = {1, 31, 33, 257};
  for (int N : ns)
    for (int mode = 0; mode < 3; ++mode)   // empty, full, random
      for (int rep = 0; rep < 3; ++rep) one_case(rng, N, mode);
  CHECK(cbv2_bm25_search_filtered(nullptr, nullptr, nullptr, 1, 1, 1, nullptr, nullptr, nullptr) == CBV2_EINVAL);
  printf("%d failed checks\n", fails);
  return fails ? 1 : 0;
}
