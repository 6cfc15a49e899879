// The (B, B) positives / negatives masks of a training batch (reference: datasets/dataset_utils.py:118-123, the collate
// function's two nested list comprehensions over `in_sorted_array`, :201-206):
//     pos_mask[i][j] = labels[j] in positives[labels[i]],        neg_mask[i][j] = labels[j] not in non_negatives[labels[i]].
// Both per-element lists are sorted (non-decreasing, repeats allowed) and arrive as CSR over the whole dataset.  One workgroup
// per batch row: the row's two lists are staged into LDS once and every label of the batch is binary-searched in them.
// Integer code only: plain loads, vector stores, one LDS atomic per wave for the optional counts.
#include "hfl_common.h"

namespace {

constexpr int BM_THREADS = 256;
// Staging capacity of EACH of the two lists, in entries: 2 x 4096 x 4 B = 32 KiB of static LDS (+ 8 B of counts), so four
// workgroups share a CU's 160 KiB.  A longer list is searched where it lies, in global memory.
constexpr int BM_LDS_ENTRIES = HFL_BATCH_MASKS_LDS_ENTRIES;

// lower bound of key in the sorted a[0..n), then equality: `in_sorted_array`.  Every lane of a workgroup searches the same
// list, so the loop runs the same number of rounds in every lane.
__device__ __forceinline__ uint32_t bm_contains(const int32_t* a, int n, int32_t key) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
    if (a[mid] < key) lo = mid + 1; else hi = mid;
  }
  return (lo < n && a[lo] == key) ? 1u : 0u;
}

// list `l` of a CSR, clamped to what an int can index; an empty list for a label outside [0, n_elems)
__device__ __forceinline__ int bm_list(const int64_t* __restrict__ off, int64_t l, int n_elems, int64_t* begin) {
  *begin = 0;
  if (l < 0 || l >= n_elems) return 0;
  const int64_t b = off[l], len = off[l + 1] - b;
  if (len <= 0) return 0;
  *begin = b;
  return len > 0x7fffffff ? 0x7fffffff : (int)len;
}

__device__ __forceinline__ void bm_stage(int32_t* __restrict__ s, const int32_t* __restrict__ g, int n) {
  if (n > BM_LDS_ENTRIES) return;
  for (int t = threadIdx.x; t < n; t += BM_THREADS) s[t] = g[t];
}

// `packed`: both masks' base addresses are congruent modulo 4, so the byte (i, j) of either sits at the same offset inside
// its dword.  Quad q of row i then covers j = 4 q - shift .. 4 q - shift + 3 with shift = (address of the row) % 4: a quad
// that lies inside the row is one aligned dword store per mask, the (at most two) quads that straddle the row's ends and
// every quad of a launch that is not `packed` are written byte by byte.
__global__ void __launch_bounds__(BM_THREADS)
batch_masks_kernel(uint8_t* __restrict__ pos_mask, uint8_t* __restrict__ neg_mask, int32_t* __restrict__ counts,
                   const int64_t* __restrict__ labels, int B, const int64_t* __restrict__ pos_off,
                   const int32_t* __restrict__ pos_idx, const int64_t* __restrict__ nn_off, const int32_t* __restrict__ nn_idx,
                   int n_elems, int packed) {
  __shared__ int32_t s_pos[BM_LDS_ENTRIES];
  __shared__ int32_t s_nn[BM_LDS_ENTRIES];
  __shared__ int32_t s_cnt[2];
  const int i = blockIdx.x;
  const int64_t own = labels[i];
  int64_t pos_b, nn_b;
  const int n_pos = bm_list(pos_off, own, n_elems, &pos_b);
  const int n_nn = bm_list(nn_off, own, n_elems, &nn_b);
  const int32_t* g_pos = pos_idx + pos_b;
  const int32_t* g_nn = nn_idx + nn_b;
  bm_stage(s_pos, g_pos, n_pos);
  bm_stage(s_nn, g_nn, n_nn);
  if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  const bool pos_lds = n_pos <= BM_LDS_ENTRIES, nn_lds = n_nn <= BM_LDS_ENTRIES;      // uniform over the workgroup

  uint8_t* prow = pos_mask + (int64_t)i * B;
  uint8_t* nrow = neg_mask + (int64_t)i * B;
  const int shift = packed ? (int)(reinterpret_cast<uintptr_t>(prow) & 3) : 0;
  const int64_t n_quads = ((int64_t)B + shift + 3) >> 2;
  int c_pos = 0, c_neg = 0;
  for (int64_t q = threadIdx.x; q < n_quads; q += BM_THREADS) {
    const int64_t j0 = 4 * q - shift;
    uint32_t pw = 0, nw = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int64_t j = j0 + c;
      if (j < 0 || j >= B) continue;
      const int64_t key64 = labels[j];
      const int32_t key = (int32_t)key64;
      uint32_t p = 0, nn = 0;
      if (key64 == (int64_t)key) {                               // every stored id is an int32: anything else is in no list
        p = pos_lds ? bm_contains(s_pos, n_pos, key) : bm_contains(g_pos, n_pos, key);
        nn = nn_lds ? bm_contains(s_nn, n_nn, key) : bm_contains(g_nn, n_nn, key);
      }
      pw |= p << (8 * c);
      nw |= (nn ^ 1u) << (8 * c);
      c_pos += (int)p;
      c_neg += (int)(nn ^ 1u);
    }
    if (packed && j0 >= 0 && j0 + 3 < B) {
      *reinterpret_cast<uint32_t*>(prow + j0) = pw;
      *reinterpret_cast<uint32_t*>(nrow + j0) = nw;
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int64_t j = j0 + c;
        if (j < 0 || j >= B) continue;
        prow[j] = (uint8_t)((pw >> (8 * c)) & 1u);
        nrow[j] = (uint8_t)((nw >> (8 * c)) & 1u);
      }
    }
  }
  if (counts == nullptr) return;                                 // uniform: a kernel argument
#pragma unroll
  for (int m = HFL_WAVE / 2; m > 0; m >>= 1) {
    c_pos += __shfl_xor(c_pos, m, HFL_WAVE);
    c_neg += __shfl_xor(c_neg, m, HFL_WAVE);
  }
  if ((threadIdx.x & (HFL_WAVE - 1)) == 0) {
    atomicAdd(&s_cnt[0], c_pos);
    atomicAdd(&s_cnt[1], c_neg);
  }
  __syncthreads();
  if (threadIdx.x < 2) counts[2 * (int64_t)i + threadIdx.x] = s_cnt[threadIdx.x];
}

}  // namespace

// 32 KiB + 8 B of static LDS: below the 64 KiB a launch may use without hipFuncSetAttribute.
extern "C" int hfl_batch_masks(uint8_t* pos_mask, uint8_t* neg_mask, int32_t* counts, const int64_t* labels, int batch,
                               const int64_t* pos_off, const int32_t* pos_idx, const int64_t* nn_off, const int32_t* nn_idx,
                               int n_elems, hfl_stream_t stream) {
  if (batch <= 0 || n_elems <= 0 || pos_mask == nullptr || neg_mask == nullptr || labels == nullptr || pos_off == nullptr ||
      pos_idx == nullptr || nn_off == nullptr || nn_idx == nullptr)
    return HFL_EINVAL;
  const int packed = ((reinterpret_cast<uintptr_t>(pos_mask) ^ reinterpret_cast<uintptr_t>(neg_mask)) & 3) == 0;
  batch_masks_kernel<<<batch, BM_THREADS, 0, static_cast<hipStream_t>(stream)>>>(
      pos_mask, neg_mask, counts, labels, batch, pos_off, pos_idx, nn_off, nn_idx, n_elems, packed);
  HFL_RETURN_LAST_ERROR();
}
