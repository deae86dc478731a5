// Level-of-detail pyramid of a PlenOctree (gfx950): pxo_tree_lod_fill (include/plenoctree_octree.h, "level of detail") writes,
// into the row of every cell that has a child, the density-weighted mean of that child's eight rows, deepest level first.
// The rows it writes are rows no renderer reads (a marcher stops at child == 0), so a full-depth render is untouched; a copy
// of `child` with the pointers of depth-L nodes zeroed renders level L from the same data.
//
// Compiled with -ffp-contract=off (plenoctree_amd/build.py): the value of a node is defined operation by operation in
// float32 (products, left-to-right sums, one IEEE division); a fused multiply-add would change the last bit.
//
// One launch per depth, max_depth .. 1, in stream order.  One lane per (node, channel): consecutive lanes read consecutive
// channels of a row, so each of the eight row loads of a wave is one run of consecutive floats (two where the wave straddles
// a node boundary); the eight sigmas are broadcast loads of lines the row loads fetch anyway.  A level reads only nodes of
// its own depth and writes only rows of nodes one level up, and every parent cell has exactly one child: no atomics, no race.
#include "pxo_common.h"
#include "../../include/plenoctree_octree.h"

namespace pxo {

constexpr int kLodBlock = 256;

// nodes are picked by their stored depth, not by their position (as tree_collapse_mark_kernel does): a tree that is not in
// level order, or one that has been collapsed, works too
__global__ void __launch_bounds__(kLodBlock)
tree_lod_fill_kernel(const int32_t* __restrict__ child, const int32_t* __restrict__ parent_depth, float* data, int64_t n,
                     int D, int d) {
  const int64_t i = blockIdx.x * (int64_t)kLodBlock + threadIdx.x;
  if (i >= n * D) return;
  const int64_t node = i / D;
  const int k = (int)(i - node * D);
  if (parent_depth[node * 2 + 1] != d) return;
  const int64_t pcell = parent_depth[node * 2];
  // the parent cell must point back at this node: a row is written only where a child pointer says it is not a leaf's
  if (pcell < 0 || pcell >= n * 8) return;
  const int skip = child[pcell];
  if (skip == 0 || (pcell >> 3) + skip != node) return;
  const float* rows = data + node * 8 * (int64_t)D;
  float w[8], c[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    w[j] = fmaxf(rows[j * D + (D - 1)], 0.0f);
    c[j] = rows[j * D + k];
  }
  float S = w[0] + w[1];
#pragma unroll
  for (int j = 2; j < 8; ++j) S = S + w[j];
  float out;
  if (k == D - 1) {
    out = S * 0.125f;
  } else if (S > 0.0f) {
    float acc = w[0] * c[0];
#pragma unroll
    for (int j = 1; j < 8; ++j) acc = acc + w[j] * c[j];
    out = acc / S;                                        // IEEE: hipcc's float division is correctly rounded
  } else {
    out = 0.0f;
  }
  data[pcell * D + k] = out;
}

}  // namespace pxo

using namespace pxo;

extern "C" int pxo_tree_lod_fill(const int32_t* child, const int32_t* parent_depth, float* data, int64_t n_internal,
                                 int data_dim, int max_depth, void* stream) {
  PXO_REQUIRE(n_internal >= 1 && n_internal < ((int64_t)1 << 28), "pxo_tree_lod_fill: n_internal %lld outside [1, 2^28)",
              (long long)n_internal);
  const int K = (data_dim - 1) / 3;
  PXO_REQUIRE(data_dim == 3 * K + 1 && (K == 1 || K == 4 || K == 9 || K == 16 || K == 25),
              "pxo_tree_lod_fill: data_dim %d is not 3 k + 1 with k in {1, 4, 9, 16, 25}", data_dim);
  PXO_REQUIRE(max_depth >= 0 && max_depth <= PXO_TREE_MAX_DEPTH, "pxo_tree_lod_fill: max_depth %d outside [0, %d]", max_depth,
              PXO_TREE_MAX_DEPTH);
  PXO_REQUIRE(child && parent_depth && data, "pxo_tree_lod_fill: null pointer");
  if (n_internal == 1 || max_depth == 0) return 0;      // a root-only tree has no cell with a child
  hipStream_t s = (hipStream_t)stream;
  const int64_t blocks = (n_internal * data_dim + kLodBlock - 1) / kLodBlock;     // < 2^28 * 76 / 256 < 2^31
  for (int d = max_depth; d >= 1; --d)
    hipLaunchKernelGGL(tree_lod_fill_kernel, dim3((unsigned)blocks), dim3(kLodBlock), 0, s, child, parent_depth, data,
                       n_internal, data_dim, d);
  return check_launch("tree_lod_fill");
}
