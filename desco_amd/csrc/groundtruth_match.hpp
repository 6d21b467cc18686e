// The match plan shared by the pattern-guided ground-truth matchers (groundtruth_match.cpp on the host,
// groundtruth_match_dev.hip on the GPU).  A plan is a flat int32 array:
//
//   plan[0] = number of queries Q, plan[1] = number of anchors A, then A records of GTM_REC int32 each, sorted by
//   query.  One record = one anchor = one orbit of the query's automorphism group: the query node (the orbit's
//   smallest) that is mapped to the root v while every other image stays below v.
//
//   rec[GTM_QUERY]       query index (the column of `out` the record counts into)
//   rec[GTM_K]           number of query nodes k, 2..16
//   rec[GTM_ANCHOR]      the anchor (= rec[GTM_NODE])
//   rec[GTM_DIVISOR]     what a count of maps is divided by to give subsets: 1, because the order constraints
//                        below leave exactly one map per subset (kept in the format so that a reader can assert it)
//   rec[GTM_NODE + i]    query node matched at position i; position 0 is the anchor, and every later node is
//                        adjacent to an earlier one (a connected matching order)
//   rec[GTM_PARENT + i]  i >= 1: the earlier position whose image's adjacency row supplies the candidates of i
//   rec[GTM_ADJ + i]     bit j (j < i): the image of i must be adjacent to the image of j; a clear bit j < i means
//                        it must NOT be (induced matching)
//   rec[GTM_LT + i]      bit j (j < i): image(i) < image(j)   } symmetry breaking (Grochow-Kellis) inside the
//   rec[GTM_GT + i]      bit j (j < i): image(i) > image(j)   } stabiliser of the anchor
//
// The LABELLED plan (desco_canonical_match_plan_labelled) is built over labelled isomorphism classes:
//
//   plan[0] = number of classes C, plan[1] = number of records A, plan[2] = number of buckets B, plan[3] = the size
//   of the largest bucket, then A records of GTML_REC int32 each, then B buckets of GTML_BUCKET int32 each.
//
//   A labelled record is the record above (rec[GTM_QUERY] = the class, one record per orbit of the LABEL-PRESERVING
//   automorphisms, LT / GT breaking only that group) followed by
//   rec[GTML_LABEL + i]  label id (>= 0) the image of position i must carry
//   The records are sorted by (rec[GTML_LABEL], rec[GTML_LABEL + 1]), then by class.  Bucket b = one run of equal
//   (label of position 0, label of position 1): bucket[0], bucket[1] = the two labels, [bucket[2], bucket[3]) = its
//   records; buckets ascend by (label 0, label 1) and tile [0, A).  A root v and its neighbour u0 can only be matched
//   by the records of bucket (label[v], label[u0]): the device launches (largest bucket) items per CSR entry.
#pragma once
#include <stdint.h>

namespace desco {

constexpr int GTM_KMAX = 16;
constexpr int GTM_HEAD = 2;
constexpr int GTM_QUERY = 0, GTM_K = 1, GTM_ANCHOR = 2, GTM_DIVISOR = 3;
constexpr int GTM_NODE = 4, GTM_PARENT = 20, GTM_ADJ = 36, GTM_LT = 52, GTM_GT = 68;
constexpr int GTM_REC = 84;
constexpr int GTML_HEAD = 4;
constexpr int GTML_LABEL = 84;
constexpr int GTML_REC = 100;
constexpr int GTML_BUCKET = 4;

// groundtruth_match.cpp: is `plan` (host memory) a well-formed plan for num_queries queries?  Both matchers index
// with its fields, so they refuse anything else.  Returns 0 or DESCO_EINVAL with the message set.
int match_plan_check(const char* who, const int32_t* plan, int64_t plan_entries, int num_queries);
// the same for a labelled plan of num_classes classes (records, labels, sort order and bucket table)
int match_plan_labelled_check(const char* who, const int32_t* plan, int64_t plan_entries, int num_classes);

}  // namespace desco
