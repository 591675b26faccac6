// densify.hip -- LoG's densification on the device: TensorTree.split_and_remove (LoG/model/tensor_tree.py:65-129),
// Splitter.split_and_remove and split_and_remove_other (LoG/model/splitter.py:138-220) without the CPU round trip.
//   * lr_launch_densify_plan     : one pass over the flag bytes (with the tree's masks of tensor_tree.py:121-122 when the
//                                  tree arrays are given), a chunked scan (the shape of counter.hip's), keep_dest[P] = the
//                                  reference's left_index; num_keep / num_split / overlap in the scratch header.
//   * lr_launch_densify_src_rows : src_row[num_keep + children * num_split], the old row behind every new row.
//   * lr_launch_move_rows        : up to 8 keys in one launch, parallel over destination words.
//   * lr_launch_split_uniform    : split_by_uniform (splitter.py:5-31, :95-130), one thread per child.
//   * lr_launch_densify_tree     : the tree buffers after split + remove (tensor_tree.py:65-118), two launches.
// Everything is streaming or gathered-row work, HBM-bound; LDS only holds block scans and a tile's row ids.
#include "common.hpp"
#include "launch.hpp"

#define DN_CHUNK 1024u
#define DN_HDR_WORDS 4u   // [0] num_keep  [1] num_split  [2] overlap (rows flagged for both while remove_split == 0)

static inline size_t dn_align4(size_t w) { return (w + 3) & ~(size_t)3; }
static inline uint32_t dn_chunks(int p) { return ((uint32_t)(p > 0 ? p : 0) + DN_CHUNK - 1) / DN_CHUNK; }
size_t lr_densify_scratch_bytes(int p) { return 4 * (DN_HDR_WORDS + 2 * dn_align4((size_t)dn_chunks(p) + 1)); }

struct DnPlanArgs {
  const uint8_t* flag_split; const uint8_t* flag_remove;
  const int32_t* node_index; const int32_t* index_parent; const int8_t* depth;   // all three or none
  uint8_t* split_out; uint8_t* remove_out;
  int32_t* keep_dest;
  uint32_t* hdr; uint32_t* chunk_keep; uint32_t* chunk_split;
  uint32_t p;
  int32_t max_level, remove_split;
};

// The flags of row i after the tree's masks: bit 0 split, bit 1 remove.
LR_DEV uint32_t dn_flags(const DnPlanArgs& a, uint32_t i) {
  bool sp = a.flag_split[i] != 0, rm = a.flag_remove[i] != 0;
  if (a.node_index) {
    const bool leaf = a.node_index[i] == -1;
    rm = rm && leaf && a.index_parent[i] != -1;           // remove &= leaf & ~root
    sp = sp && leaf && (int32_t)a.depth[i] < a.max_level;   // split &= leaf & depth < max_level
  }
  return (sp ? 1u : 0u) | (rm ? 2u : 0u);
}

__global__ void __launch_bounds__(256)
dn_count_kernel(DnPlanArgs a) {
  __shared__ uint32_t wk[4], ws[4], wo[4];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t nchunks = (a.p + DN_CHUNK - 1) / DN_CHUNK;
  for (uint32_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
    uint32_t ck = 0, cs = 0, co = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const uint32_t i = chunk * DN_CHUNK + (uint32_t)k * 256u + threadIdx.x;
      const bool in = i < a.p;
      const uint32_t f = in ? dn_flags(a, i) : 0u;
      const bool sp = f & 1u, rm = f & 2u;
      if (in) { a.split_out[i] = sp ? 1 : 0; a.remove_out[i] = rm ? 1 : 0; }
      const bool keep = in && !(rm || (a.remove_split && sp));
      ck += (uint32_t)__popcll(__ballot(keep));
      cs += (uint32_t)__popcll(__ballot(sp));
      co += (uint32_t)__popcll(__ballot(sp && rm && !a.remove_split));
    }
    if (lane == 0) { wk[wave] = ck; ws[wave] = cs; wo[wave] = co; }
    __syncthreads();
    if (threadIdx.x == 0) {
      a.chunk_keep[chunk] = wk[0] + wk[1] + wk[2] + wk[3];
      a.chunk_split[chunk] = ws[0] + ws[1] + ws[2] + ws[3];
      const uint32_t o = wo[0] + wo[1] + wo[2] + wo[3];
      if (o) atomicAdd(&a.hdr[2], o);
    }
    __syncthreads();
  }
}

// Exclusive scan of both chunk tables by one workgroup, 1024 chunks a round with a carry (any number of chunks).
__global__ void __launch_bounds__(1024)
dn_scan_kernel(uint32_t* __restrict__ chunk_keep, uint32_t* __restrict__ chunk_split, uint32_t nchunks,
               uint32_t* __restrict__ hdr) {
  __shared__ uint32_t wk[2][16];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t carry[2] = {0, 0};
  for (uint32_t base = 0; base < nchunks; base += 1024u) {
    const uint32_t i = base + threadIdx.x;
    uint32_t k[2], ik[2];
    k[0] = i < nchunks ? chunk_keep[i] : 0u;
    k[1] = i < nchunks ? chunk_split[i] : 0u;
#pragma unroll
    for (int t = 0; t < 2; t++) {
      ik[t] = k[t];
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const uint32_t u = __shfl_up(ik[t], d);
        if ((int)lane >= d) ik[t] += u;
      }
      if (lane == 63u) wk[t][wave] = ik[t];
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < 2; t++) {
      uint32_t off = 0, tot = 0;
#pragma unroll
      for (uint32_t w = 0; w < 16u; w++) {
        const uint32_t v = wk[t][w];
        if (w < wave) off += v;
        tot += v;
      }
      if (i < nchunks) (t ? chunk_split : chunk_keep)[i] = carry[t] + off + ik[t] - k[t];
      carry[t] += tot;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) { hdr[0] = carry[0]; hdr[1] = carry[1]; }
}

// Ranks of a chunk's rows among the kept / the split rows.  WHAT = 0: keep_dest (the plan).  WHAT = 1: src_row (after
// the counts were read): a kept row's slot holds its old row, the `children` slots of the k-th split row hold that row.
template <int WHAT>
__global__ void __launch_bounds__(256)
dn_emit_kernel(const uint8_t* __restrict__ split, const uint8_t* __restrict__ remove, uint32_t p, int32_t remove_split,
               const uint32_t* __restrict__ chunk_keep, const uint32_t* __restrict__ chunk_split,
               int32_t* __restrict__ keep_dest, int32_t* __restrict__ src_row, uint32_t num_keep, uint32_t num_split,
               uint32_t children) {
  __shared__ uint32_t cntk[16], cnts[16];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint64_t below = (1ull << lane) - 1ull;
  const uint32_t nchunks = (p + DN_CHUNK - 1) / DN_CHUNK;
  for (uint32_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
    bool keep[4], sp[4];
    uint64_t bk[4], bs[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const uint32_t i = chunk * DN_CHUNK + (uint32_t)k * 256u + threadIdx.x;
      const bool in = i < p;
      sp[k] = in && split[i] != 0;
      keep[k] = in && !(remove[i] != 0 || (remove_split && sp[k]));
      bk[k] = __ballot(keep[k]);
      bs[k] = __ballot(sp[k]);
      if (lane == 0) { cntk[k * 4 + wave] = (uint32_t)__popcll(bk[k]); cnts[k * 4 + wave] = (uint32_t)__popcll(bs[k]); }
    }
    __syncthreads();
    uint32_t prek = chunk_keep[chunk], pres = chunk_split[chunk], e = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      for (; e < (uint32_t)k * 4u + wave; e++) { prek += cntk[e]; pres += cnts[e]; }
      const uint32_t i = chunk * DN_CHUNK + (uint32_t)k * 256u + threadIdx.x;
      const uint32_t rk = prek + (uint32_t)__popcll(bk[k] & below);
      const uint32_t rs = pres + (uint32_t)__popcll(bs[k] & below);
      if (WHAT == 0) {
        if (i < p) keep_dest[i] = keep[k] ? (int32_t)rk : -1;
      } else {
        if (keep[k] && rk < num_keep) src_row[rk] = (int32_t)i;
        if (sp[k] && rs < num_split)
          for (uint32_t j = 0; j < children; j++) src_row[(size_t)num_keep + (size_t)children * rs + j] = (int32_t)i;
      }
    }
    __syncthreads();
  }
}

hipError_t lr_launch_densify_plan(int p, const uint8_t* flag_split, const uint8_t* flag_remove, int remove_split,
                                  const int32_t* node_index, const int32_t* index_parent, const int8_t* depth,
                                  int max_level, uint8_t* split_out, uint8_t* remove_out, int32_t* keep_dest,
                                  void* scratch, hipStream_t s) {
  uint32_t* w = reinterpret_cast<uint32_t*>(scratch);
  const uint32_t nchunks = dn_chunks(p);
  DnPlanArgs a;
  a.flag_split = flag_split; a.flag_remove = flag_remove;
  a.node_index = node_index; a.index_parent = index_parent; a.depth = depth;
  a.split_out = split_out; a.remove_out = remove_out; a.keep_dest = keep_dest;
  a.hdr = w; a.chunk_keep = w + DN_HDR_WORDS; a.chunk_split = a.chunk_keep + dn_align4((size_t)nchunks + 1);
  a.p = (uint32_t)p; a.max_level = max_level; a.remove_split = remove_split ? 1 : 0;
  hipError_t e = hipMemsetAsync(w, 0, 4 * DN_HDR_WORDS, s);
  if (e != hipSuccess) return e;
  if (!nchunks) return hipSuccess;
  lr_prof_begin(LRK_MISC, s);
  const uint32_t g = nchunks > 4096u ? 4096u : nchunks;
  hipLaunchKernelGGL(dn_count_kernel, dim3(g), dim3(256), 0, s, a);
  hipLaunchKernelGGL(dn_scan_kernel, dim3(1), dim3(1024), 0, s, a.chunk_keep, a.chunk_split, nchunks, a.hdr);
  hipLaunchKernelGGL(dn_emit_kernel<0>, dim3(g), dim3(256), 0, s, (const uint8_t*)split_out, (const uint8_t*)remove_out,
                     a.p, a.remove_split, (const uint32_t*)a.chunk_keep, (const uint32_t*)a.chunk_split, keep_dest,
                     (int32_t*)nullptr, 0u, 0u, 0u);
  lr_prof_end(LRK_MISC, s);
  return hipGetLastError();
}

hipError_t lr_launch_densify_src_rows(int p, int children, int remove_split, const uint8_t* split, const uint8_t* remove,
                                      int num_keep, int num_split, int32_t* src_row, const void* scratch, hipStream_t s) {
  const uint32_t nchunks = dn_chunks(p);
  if (!nchunks || num_keep + num_split == 0) return hipSuccess;
  const uint32_t* w = reinterpret_cast<const uint32_t*>(scratch);
  const uint32_t* chunk_keep = w + DN_HDR_WORDS;
  const uint32_t* chunk_split = chunk_keep + dn_align4((size_t)nchunks + 1);
  lr_prof_begin(LRK_MISC, s);
  const uint32_t g = nchunks > 4096u ? 4096u : nchunks;
  hipLaunchKernelGGL(dn_emit_kernel<1>, dim3(g), dim3(256), 0, s, split, remove, (uint32_t)p, remove_split ? 1 : 0,
                     chunk_keep, chunk_split, (int32_t*)nullptr, src_row, (uint32_t)num_keep, (uint32_t)num_split,
                     (uint32_t)children);
  lr_prof_end(LRK_MISC, s);
  return hipGetLastError();
}

// ---- row move ------------------------------------------------------------------------------------------------------
// A workgroup takes a tile of consecutive destination rows (a multiple of 16 rows, so the tile starts on a 16-byte word of
// dst), reads the tile's src_row entries once into LDS, and its threads walk the tile's 16-byte destination words.
// Compaction keeps the order, so the sources of neighbouring words are neighbours except where rows were dropped.
// A row size that is a multiple of 16 bytes (and a 16-byte aligned src) loads a word in one piece; otherwise the word is
// put together from the row's largest power-of-two unit (4 B for 12 / 36 / 180-byte rows) and stored in one piece.
// Rows >= num_keep: COPY_PARENT reads src_row like a kept row, ZERO writes zeros, SKIP leaves them to another kernel.
#define DN_TILE_WIDE 256u      // rows per tile, row size >= 16 B
#define DN_TILE_NARROW 1024u   // rows per tile below that

template <int UNIT> struct DnUnit;
template <> struct DnUnit<1> { typedef uint8_t T; };
template <> struct DnUnit<2> { typedef uint16_t T; };
template <> struct DnUnit<4> { typedef uint32_t T; };

template <int UNIT>
LR_DEV void dn_move_tile(const MoveKey& k, const int32_t* srow, uint32_t tile_rows, uint64_t tile_byte0, uint32_t tile_bytes,
                         uint32_t src_rows) {
  typedef typename DnUnit<UNIT>::T U;
  constexpr int N = 16 / UNIT;
  const uint32_t rb = k.row_bytes;
  const uint8_t* src = reinterpret_cast<const uint8_t*>(k.src);
  uint8_t* dst = reinterpret_cast<uint8_t*>(k.dst) + tile_byte0;
  for (uint32_t b = threadIdx.x * 16u; b < tile_bytes; b += 256u * 16u) {
    uint32_t row = b / rb, col = b - row * rb;
    union { uint4 v; U u[N]; } w;
    w.v = make_uint4(0, 0, 0, 0);
    if (k.vec16) {            // rb % 16 == 0: the word lies in one row, 16-byte aligned on both sides
      const int32_t sr = row < tile_rows ? srow[row] : -1;
      if (sr >= 0 && (uint32_t)sr < src_rows) w.v = *reinterpret_cast<const uint4*>(src + (size_t)sr * rb + col);
    } else {
#pragma unroll
      for (int j = 0; j < N; j++) {
        if (b + (uint32_t)j * UNIT < tile_bytes) {
          const int32_t sr = srow[row];
          if (sr >= 0 && (uint32_t)sr < src_rows) w.u[j] = *reinterpret_cast<const U*>(src + (size_t)sr * rb + col);
        }
        col += UNIT;
        if (col == rb) { col = 0; row++; }
      }
    }
    if (b + 16u <= tile_bytes) {
      *reinterpret_cast<uint4*>(dst + b) = w.v;
    } else {                  // the last word of the moved range: only the units inside it
#pragma unroll
      for (int j = 0; j < N; j++)
        if (b + (uint32_t)j * UNIT < tile_bytes) *reinterpret_cast<U*>(dst + b + j * UNIT) = w.u[j];
    }
  }
}

__global__ void __launch_bounds__(256)
dn_move_kernel(MoveArgs a) {
  __shared__ int32_t srow[DN_TILE_NARROW];
  const MoveKey& k = a.key[blockIdx.y];
  const uint32_t rows = k.child_mode == LR_MOVE_SKIP ? (uint32_t)a.num_keep : (uint32_t)a.num_new;
  const uint32_t tr = k.row_bytes >= 16u ? DN_TILE_WIDE : DN_TILE_NARROW;
  const uint32_t tiles = (rows + tr - 1) / tr;
  for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const uint32_t r0 = tile * tr;
    const uint32_t n = rows - r0 < tr ? rows - r0 : tr;
    for (uint32_t r = threadIdx.x; r < n; r += 256u) {
      const uint32_t d = r0 + r;
      srow[r] = (d >= (uint32_t)a.num_keep && k.child_mode == LR_MOVE_ZERO) ? -1 : a.src_row[d];
    }
    __syncthreads();
    const uint64_t byte0 = (uint64_t)r0 * k.row_bytes;
    const uint32_t bytes = n * k.row_bytes;
    if (k.unit == 4) dn_move_tile<4>(k, srow, n, byte0, bytes, (uint32_t)a.src_rows);
    else if (k.unit == 2) dn_move_tile<2>(k, srow, n, byte0, bytes, (uint32_t)a.src_rows);
    else dn_move_tile<1>(k, srow, n, byte0, bytes, (uint32_t)a.src_rows);
    __syncthreads();
  }
}

hipError_t lr_launch_move_rows(const MoveArgs& a, int num_keys, hipStream_t s) {
  if (num_keys <= 0 || a.num_new <= 0) return hipSuccess;
  uint32_t tiles = 1;
  for (int i = 0; i < num_keys; i++) {
    const uint32_t tr = a.key[i].row_bytes >= 16u ? DN_TILE_WIDE : DN_TILE_NARROW;
    const uint32_t t = ((uint32_t)a.num_new + tr - 1) / tr;
    tiles = t > tiles ? t : tiles;
  }
  if (tiles > 16384u) tiles = 16384u;
  lr_prof_begin(LRK_MISC, s);
  hipLaunchKernelGGL(dn_move_kernel, dim3(tiles, (uint32_t)num_keys), dim3(256), 0, s, a);
  lr_prof_end(LRK_MISC, s);
  return hipGetLastError();
}

// ---- uniform split (splitter.py:5-31, :95-130) ---------------------------------------------------------------------
// One thread per child.  The children of one parent share their scales in every round (both halves get the same
// scale[axis] * factor), so each child repeats the parent's rounds and takes its own side: bit (rounds - 1 - r) of the
// child's number is the side of round r (parent-major, then --, -+, +-, ++).  The operations are the reference's, one by
// one and uncontracted: exp, the rotation of the raw quaternion divided by its norm (geometry.py:4-25), per round the
// longest axis of the CURRENT scales (ties to the lowest axis, as torch.max on the CPU), centre + R[:, axis] * (+-0.5 *
// scale[axis]), scale[axis] *= factor; then log of all three scales.
__global__ void __launch_bounds__(256)
dn_split_kernel(int32_t num_keep, int32_t num_split, int32_t children, int32_t rounds, float factor, int32_t src_rows,
                const int32_t* __restrict__ src_row, const float* __restrict__ xyz, const float* __restrict__ scaling,
                const float* __restrict__ rotation, float* __restrict__ xyz_new, float* __restrict__ scaling_new) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (int64_t)num_split * children) return;
  const size_t d = (size_t)num_keep + (size_t)t;
  const int32_t j = (int32_t)(t % children);
  const int32_t sr = src_row[d];
  if (sr < 0 || sr >= src_rows) return;
  float sc[3], c[3], q[4];
#pragma unroll
  for (int i = 0; i < 3; i++) { sc[i] = expf(scaling[3 * (size_t)sr + i]); c[i] = xyz[3 * (size_t)sr + i]; }
#pragma unroll
  for (int i = 0; i < 4; i++) q[i] = rotation[4 * (size_t)sr + i];
  const float norm = __fsqrt_rn(__fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(q[0], q[0]), __fmul_rn(q[1], q[1])),
                                                    __fmul_rn(q[2], q[2])), __fmul_rn(q[3], q[3])));
  const float r = __fdiv_rn(q[0], norm), x = __fdiv_rn(q[1], norm), y = __fdiv_rn(q[2], norm), z = __fdiv_rn(q[3], norm);
  float R[9];
#define DN_M(a, b) __fmul_rn(a, b)
  R[0] = __fsub_rn(1.f, __fmul_rn(2.f, __fadd_rn(DN_M(y, y), DN_M(z, z))));
  R[1] = __fmul_rn(2.f, __fsub_rn(DN_M(x, y), DN_M(r, z)));
  R[2] = __fmul_rn(2.f, __fadd_rn(DN_M(x, z), DN_M(r, y)));
  R[3] = __fmul_rn(2.f, __fadd_rn(DN_M(x, y), DN_M(r, z)));
  R[4] = __fsub_rn(1.f, __fmul_rn(2.f, __fadd_rn(DN_M(x, x), DN_M(z, z))));
  R[5] = __fmul_rn(2.f, __fsub_rn(DN_M(y, z), DN_M(r, x)));
  R[6] = __fmul_rn(2.f, __fsub_rn(DN_M(x, z), DN_M(r, y)));
  R[7] = __fmul_rn(2.f, __fadd_rn(DN_M(y, z), DN_M(r, x)));
  R[8] = __fsub_rn(1.f, __fmul_rn(2.f, __fadd_rn(DN_M(x, x), DN_M(y, y))));
#undef DN_M
  for (int32_t rd = 0; rd < rounds; rd++) {
    int axis = 0;
    float m = sc[0];
    if (sc[1] > m) { axis = 1; m = sc[1]; }
    if (sc[2] > m) { axis = 2; m = sc[2]; }
    const float side = ((j >> (rounds - 1 - rd)) & 1) ? 0.5f : -0.5f;
    const float off = __fmul_rn(side, m);
#pragma unroll
    for (int i = 0; i < 3; i++) {
      const float col = axis == 0 ? R[3 * i] : (axis == 1 ? R[3 * i + 1] : R[3 * i + 2]);
      c[i] = __fadd_rn(__fmul_rn(col, off), c[i]);
    }
    const float ns = __fmul_rn(m, factor);
    if (axis == 0) sc[0] = ns; else if (axis == 1) sc[1] = ns; else sc[2] = ns;
  }
#pragma unroll
  for (int i = 0; i < 3; i++) { xyz_new[3 * d + i] = c[i]; scaling_new[3 * d + i] = logf(sc[i]); }
}

hipError_t lr_launch_split_uniform(int num_keep, int num_split, int children, float factor, int src_rows,
                                   const int32_t* src_row, const float* xyz, const float* scaling, const float* rotation,
                                   float* xyz_new, float* scaling_new, hipStream_t s) {
  const int64_t total = (int64_t)num_split * children;
  if (total <= 0) return hipSuccess;
  const int rounds = children == 2 ? 1 : (children == 4 ? 2 : 3);
  lr_prof_begin(LRK_MISC, s);
  hipLaunchKernelGGL(dn_split_kernel, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, s, num_keep, num_split, children,
                     rounds, factor, src_rows, src_row, xyz, scaling, rotation, xyz_new, scaling_new);
  lr_prof_end(LRK_MISC, s);
  return hipGetLastError();
}

// ---- tree (tensor_tree.py:65-118) ----------------------------------------------------------------------------------
// Threads [0, num_new): the per-point arrays of new row d.  A kept row copies its old row with index_parent sent through
// keep_dest; child j of the k-th split row gets keep_dest[parent], j, depth + 1 and no node, and child 0 also gives its
// parent the node num_nodes + k (a split row is a leaf, so nothing else writes that slot).
// Threads [num_new, num_new + (num_nodes + num_split) * children): the tree entries; old ones through keep_dest (a removed
// child becomes -1), row num_nodes + k holds num_keep + children * k + j.
__global__ void __launch_bounds__(256)
dn_tree_kernel(TreeArgs a) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t num_new = (int64_t)a.num_keep + (int64_t)a.num_split * a.children;
  if (t < num_new) {
    const int32_t sr = a.src_row[t];
    if (sr < 0 || sr >= a.p) return;
    if (t < a.num_keep) {
      if (!a.split[sr]) a.node_index_new[t] = a.node_index[sr];
      const int32_t ip = a.index_parent[sr];
      a.index_parent_new[t] = (ip >= 0 && ip < a.p) ? a.keep_dest[ip] : -1;
      a.local_index_new[t] = a.local_index[sr];
      a.depth_new[t] = a.depth[sr];
    } else {
      const int64_t c = t - a.num_keep;
      const int32_t k = (int32_t)(c / a.children), j = (int32_t)(c - (int64_t)k * a.children);
      const int32_t pd = a.keep_dest[sr];
      a.node_index_new[t] = -1;
      a.index_parent_new[t] = pd;
      a.local_index_new[t] = (int8_t)j;
      a.depth_new[t] = (int8_t)(a.depth[sr] + 1);
      if (j == 0 && pd >= 0 && pd < a.num_keep) a.node_index_new[pd] = a.num_nodes + k;
    }
    return;
  }
  const int64_t e = t - num_new;
  const int64_t old_entries = (int64_t)a.num_nodes * a.children;
  if (e < old_entries) {
    const int32_t v = a.tree[e];
    a.tree_new[e] = (v >= 0 && v < a.p) ? a.keep_dest[v] : -1;
  } else if (e < old_entries + (int64_t)a.num_split * a.children) {
    a.tree_new[e] = (int32_t)(a.num_keep + (e - old_entries));
  }
}

// Second pass, on the finished tree rows: a point whose node has no entry >= 0 left is a leaf again (:115-118), parents
// orphaned in earlier calls included; their tree rows stay.
__global__ void __launch_bounds__(256)
dn_tree_orphan_kernel(TreeArgs a) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (int64_t)a.num_keep) return;        // children are leaves already
  const int32_t node = a.node_index_new[t];
  if (node < 0 || node >= a.num_nodes + a.num_split) return;
  bool any = false;
  for (int32_t j = 0; j < a.children; j++) any = any || a.tree_new[(size_t)node * a.children + j] >= 0;
  if (!any) a.node_index_new[t] = -1;
}

hipError_t lr_launch_densify_tree(const TreeArgs& a, hipStream_t s) {
  const int64_t num_new = (int64_t)a.num_keep + (int64_t)a.num_split * a.children;
  const int64_t total = num_new + ((int64_t)a.num_nodes + a.num_split) * a.children;
  if (total <= 0) return hipSuccess;
  lr_prof_begin(LRK_MISC, s);
  hipLaunchKernelGGL(dn_tree_kernel, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, s, a);
  if (a.num_keep > 0)
    hipLaunchKernelGGL(dn_tree_orphan_kernel, dim3((uint32_t)(((int64_t)a.num_keep + 255) / 256)), dim3(256), 0, s, a);
  lr_prof_end(LRK_MISC, s);
  return hipGetLastError();
}
