// cbv2_groups_build_host: the host half of a grouping (include/colbert_mi355x.h,
// "Grouped search").  A stable counting sort of the shard's member chunks by
// group: the members of one group become one contiguous segment of `order`,
// ascending chunk id inside it, segments in ascending group index; groups
// without members take no segment.  cbv2_groups_create uploads the result; the
// device kernels never see the caller's group_of array.
#include <cstdint>
#include <cstdio>
#include <new>
#include <vector>

#include "colbert_mi355x.h"

extern "C" int cbv2_set_error(int code, const char* msg);  // colbert_mi355x.hip

extern "C" {

int cbv2_groups_build_host(const int32_t* group_of, int64_t n, int32_t G, int32_t* order, int32_t* offsets,
                           int32_t* labels, int64_t* out3) {
  if (!(n >= 0 && n <= 0x7fffffffLL)) return cbv2_set_error(CBV2_EINVAL, "n must be in [0, 2^31 - 1]");
  if (G < 1) return cbv2_set_error(CBV2_EINVAL, "G must be >= 1");
  if (!offsets || !labels || !out3 || (n > 0 && (!group_of || !order)))
    return cbv2_set_error(CBV2_EINVAL, "null pointer");
  std::vector<int32_t> cnt;
  try {
    cnt.assign((size_t)G, 0);
  } catch (const std::bad_alloc&) {
    return cbv2_set_error(CBV2_EINVAL, "G too large for the host's memory");
  }
  // validate everything before the first write: an error leaves every output as it was
  int64_t members = 0;
  for (int64_t i = 0; i < n; ++i) {
    const int32_t g = group_of[i];
    if (g < -1 || g >= G) {
      char msg[160];
      snprintf(msg, sizeof(msg), "group_of[%lld] = %d is outside [-1, %d)", (long long)i, g, G);
      return cbv2_set_error(CBV2_EINVAL, msg);
    }
    if (g >= 0) {
      ++cnt[(size_t)g];
      ++members;
    }
  }
  // segment bounds over the groups that have members; cnt[g] becomes the next free slot of group g
  int64_t groups = 0, largest = 0;
  int32_t at = 0;
  for (int32_t g = 0; g < G; ++g) {
    const int32_t c = cnt[(size_t)g];
    if (c == 0) continue;
    offsets[groups] = at;
    labels[groups] = g;
    ++groups;
    if (c > largest) largest = c;
    cnt[(size_t)g] = at;
    at += c;
  }
  offsets[groups] = at;
  for (int64_t i = 0; i < n; ++i) {   // ascending i: ascending chunk id inside every segment
    const int32_t g = group_of[i];
    if (g >= 0) order[cnt[(size_t)g]++] = (int32_t)i;
  }
  out3[0] = members;
  out3[1] = groups;
  out3[2] = largest;
  return CBV2_OK;
}

}  // extern "C"
