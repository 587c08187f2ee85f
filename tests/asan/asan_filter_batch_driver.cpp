// AddressSanitizer / UBSan driver for the per-query filtered host BM25
// (cbv2_bm25_search_filtered_batch): a batch whose queries hold an empty, a
// full, a single-doc and random bitmaps and NULL entries, on corpora whose
// last bitmap word is partial (n = 1, 31, 33, 257, 501), k above some allowed
// counts, 1 and 4 threads.  Every row must equal cbv2_bm25_search_filtered on
// that query alone (cbv2_bm25_search for a NULL entry), ids and score bits.
// Each bitmap is its own heap block of exactly ceil(n / 32) words, so a read
// past one, or through the wrong row's pointer, is an ASan report.  Built by
// tests/test_filter_batch_host.py with g++ -fsanitize=address,undefined;
// test infrastructure only (no GPU code, no Python).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

static void one_case(std::mt19937& rng, int N) {
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
  const int B = 7;   // modes: empty, full, one doc, NULL, random, NULL, random
  const int nw = (N + 31) / 32;
  std::vector<std::vector<uint32_t>> maps(B);
  std::vector<const uint32_t*> allows(B, nullptr);
  for (int b = 0; b < B; ++b) {
    if (b == 3 || b == 5) continue;
    maps[b].assign(nw, 0u);
    for (int d = 0; d < N; ++d) {
      const bool ok = b == 0 ? false : b == 1 ? true : b == 2 ? d == N / 2 : rng() % 3 == 0;
      if (ok) maps[b][d >> 5] |= 1u << (d & 31);
    }
    if (N & 31) maps[b][nw - 1] |= ~0u << (N & 31);   // garbage past N
    allows[b] = maps[b].data();
  }
  std::vector<int64_t> qo(B + 1, 0);
  std::vector<int32_t> qt;
  for (int b = 0; b < B; ++b) {
    const int ql = b == 4 ? 0 : 1 + rng() % 5;   // one query without terms: padding only
    for (int j = 0; j < ql; ++j) qt.push_back((int32_t)(rng() % (V + 2)) - 1);   // out-of-range ids too
    qo[b + 1] = (int64_t)qt.size();
  }
  const int32_t* qp = qt.empty() ? nullptr : qt.data();
  const int ks[3] = {1, N / 3 + 1, N + 5};
  for (int k : ks) {
    for (int threads : {1, 4}) {
      std::vector<int32_t> ids((size_t)B * k, -7), want_i(k);
      std::vector<float> sc((size_t)B * k, -7.0f), want_s(k);
      CHECK(cbv2_bm25_search_filtered_batch(ix, qp, qo.data(), B, k, threads, allows.data(), ids.data(), sc.data()) ==
            CBV2_OK);
      for (int b = 0; b < B; ++b) {   // query b alone (its CSR slice), under its own bitmap
        const int64_t one[2] = {0, qo[b + 1] - qo[b]};
        const int32_t* q1 = qp ? qp + qo[b] : nullptr;
        if (allows[b])
          CHECK(cbv2_bm25_search_filtered(ix, q1, one, 1, k, 1, allows[b], want_i.data(), want_s.data()) == CBV2_OK);
        else
          CHECK(cbv2_bm25_search(ix, q1, one, 1, k, 1, want_i.data(), want_s.data()) == CBV2_OK);
        CHECK(memcmp(want_i.data(), ids.data() + (size_t)b * k, sizeof(int32_t) * k) == 0);
        CHECK(memcmp(want_s.data(), sc.data() + (size_t)b * k, sizeof(float) * k) == 0);
      }
      // scores are optional
      CHECK(cbv2_bm25_search_filtered_batch(ix, qp, qo.data(), B, k, threads, allows.data(), ids.data(), nullptr) ==
            CBV2_OK);
    }
  }
  cbv2_bm25_destroy(ix);
}

int main() {
  std::mt19937 rng(4321);
  const int ns[5] = {1, 31, 33, 257, 501};
  for (int N : ns)
    for (int rep = 0; rep < 2; ++rep) one_case(rng, N);
  int32_t id = 0;
  const int64_t qo[2] = {0, 0};
  const uint32_t* none[1] = {nullptr};
  CHECK(cbv2_bm25_search_filtered_batch(nullptr, nullptr, qo, 1, 1, 1, none, &id, nullptr) == CBV2_EINVAL);
  printf("%d failed checks\n", fails);
  return fails ? 1 : 0;
}
