// The statistic-set tables of the BatchNorm kernels (batchnorm.hip, bn_precise.hip) and the argument test of their entry points.
#pragma once
#include <stdint.h>
#include <initializer_list>
#include "common.h"

#define UTV2_BN_MAX_SETS 16
#define BN_CHUNK 64      // rows per stage-1 block

struct BnSets {
  int n;
  int row0[UTV2_BN_MAX_SETS];    // first row of the set
  int rows[UTV2_BN_MAX_SETS];    // its row count
  int level[UTV2_BN_MAX_SETS];   // row of the [L, C] parameter / running-statistics matrices it uses
  int chunk0[UTV2_BN_MAX_SETS + 1];  // first chunk of the set; [n] = number of chunks
};

static inline int bn_chunks_of(int rows) { return (rows + BN_CHUNK - 1) / BN_CHUNK; }
// Host tables -> the kernel argument.  `rows` is always needed (it defines the chunks); `need` says which other tables the entry's
// kernels use: BN_ROW0 when they place rows in the activation, BN_LEVEL when they touch a per-level matrix.  What is needed must be
// given and is validated (rows inside [0, P), levels inside [0, nlevels)); what is not needed is not read, zero in `st` and unused.
enum { BN_ROWS_ONLY = 0, BN_ROW0 = 1, BN_LEVEL = 2 };
static inline int bn_fill_sets(BnSets& st, int need, int nsets, const int* row0, const int* rows, const int* level, int nlevels, int64_t P) {
  const bool pos = need & BN_ROW0, lev = need & BN_LEVEL;
  if (nsets < 1 || nsets > UTV2_BN_MAX_SETS || !rows || (pos && !row0) || (lev && !level)) return UTV2_EARG;
  st.n = nsets;
  int c = 0;
  for (int s = 0; s < nsets; ++s) {
    if (rows[s] < 1 || (pos && (row0[s] < 0 || (int64_t)row0[s] + rows[s] > P)) || (lev && (level[s] < 0 || level[s] >= nlevels))) return UTV2_EARG;
    st.row0[s] = pos ? row0[s] : 0, st.rows[s] = rows[s], st.level[s] = lev ? level[s] : 0;
    st.chunk0[s] = c;
    c += bn_chunks_of(rows[s]);
  }
  st.chunk0[nsets] = c;
  return UTV2_OK;
}

// The argument test of every entry.  Every pointer non-null; BN_F32Q ones (fp32 read as quads) 16-byte aligned, BN_ACTQ ones (quads of
// the activation type `dtype`) 8 or 16 bytes.  C: whole quads when the entry's kernels walk quads, else >= 1.  Then the set tables -> st.
enum BnAlign { BN_ANY, BN_F32Q, BN_ACTQ };
struct BnPtr { const void* p; BnAlign a; };
static inline int bn_gate(BnSets& st, int need, int nsets, const int* row0, const int* rows, const int* level, int nlevels, int64_t P,
                   std::initializer_list<BnPtr> ptrs, int dtype, int C, bool quads) {
  for (const BnPtr& q : ptrs) {
    if (!q.p || ((uintptr_t)q.p & (q.a == BN_ANY ? 0 : (q.a == BN_ACTQ && dtype == UTV2_BF16) ? 7 : 15))) return UTV2_EARG;
  }
  if (quads ? (C < 4 || (C & 3)) : C < 1) return UTV2_EARG;
  return bn_fill_sets(st, need, nsets, row0, rows, level, nlevels, P);
}
