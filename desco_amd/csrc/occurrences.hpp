// Shared by the occurrence listers (desco_list_occurrences in groundtruth_match.cpp, where the host matcher lives, and
// occurrences_dev.hip on the GPU).
#pragma once
#include <stdint.h>

namespace desco {

// groundtruth_match.cpp: is `plan` (host memory) a well-formed matcher plan of exactly ONE query whose records each carry a
// permutation of the query's nodes (rec[GTM_NODE + i], i < k: the listers store column rec[GTM_NODE + i] of a row) with
// the anchor at position 0?  Returns 0 or DESCO_EINVAL with the message set.
int list_plan_check(const char* who, const int32_t* plan, int64_t plan_entries);

}  // namespace desco
