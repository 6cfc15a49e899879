// Fixed-radius join of 2-D positions in float64: which database scans lie within r_a / r_b of each query scan.  This is the
// work of the reference's tuple and test-set generators (datasets/*/generate_training_tuples*.py, generate_test_sets.py,
// datasets/CSWildPlaces/generate_train_test_tuples.py): a sklearn KDTree, `query_radius` at pos_thresh and neg_thresh, and a
// per-anchor loop of np.setdiff1d / np.sort.  Membership is what `query_radius` evaluates for the Euclidean metric, the
// reduced distance against r * r:
//     dx * dx + dy * dy <= r * r,       every operation rounded to float64 (no FMA contraction),
// (this file is compiled with -ffp-contract=off, build.EXTRA_FLAGS: the _rn intrinsics alone still fuse into v_fmac_f64),
// so the numpy restatement (tuples.radius_lists_host) gives the same bits.  float64 because UTM northings are ~6.9e6, where
// one fp32 ulp is half a metre.
//
// A tiled all-pairs scan: one wave per query row, RL_ROWS rows per workgroup sharing database tiles of RL_TILE positions
// staged in LDS as float64 pairs.  Lane l of a wave tests id tile_base + 64 s + l; a wave ballot gives the count by popcount
// and, in the fill pass, each hit's slot as the row's running base plus the popcount of the lower lanes, so every list is
// strictly ascending with no sort and no atomics (two runs give the same bits).  One distance serves both radii.  Two passes
// over one body: the count pass writes (Q, 2) int32 counts, the host makes int64 offsets of them, the fill pass writes int32
// ids.  Plain loads, vector stores.
#include "hfl_common.h"

namespace {

constexpr int RL_ROWS = HFL_RADIUS_ROWS;                         // query rows (= waves) of a workgroup
constexpr int RL_TILE = HFL_RADIUS_TILE;                         // database positions of an LDS tile
constexpr int RL_THREADS = RL_ROWS * HFL_WAVE;
static_assert(RL_TILE % HFL_WAVE == 0, "a tile is whole wave steps");
// 2048 x 16 B = 32 KiB of static LDS: five workgroups fit a CU's 160 KiB, the 32-waves-per-CU cap admits four of 8 waves.
static_assert(RL_TILE * 16 * 2 <= 160 * 1024, "at least two workgroups per CU");

template <bool FILL>
__global__ void __launch_bounds__(RL_THREADS)
radius_lists_kernel(int32_t* __restrict__ counts, int32_t* __restrict__ ids_a, int32_t* __restrict__ ids_b,
                    const int64_t* __restrict__ off_a, const int64_t* __restrict__ off_b, const double* __restrict__ queries,
                    int64_t n_queries, const double* __restrict__ database, int64_t n_database, double ra2, double rb2,
                    int exclude_self) {
  __shared__ double2 s_db[RL_TILE];
  const int lane = threadIdx.x & (HFL_WAVE - 1), wave = threadIdx.x >> 6;
  const int64_t i = (int64_t)blockIdx.x * RL_ROWS + wave;
  const bool row = i < n_queries;                                // uniform over the wave
  double qx = 0.0, qy = 0.0;
  if (row) { qx = queries[2 * i]; qy = queries[2 * i + 1]; }
  const int64_t self = exclude_self ? i : -1;
  const uint64_t below = (1ull << lane) - 1ull;                  // the lanes under this one
  // fill pass: where the row's next hit goes and where its list ends (a hit past the end is dropped, never written)
  int64_t at_a = 0, end_a = 0, at_b = 0, end_b = 0;
  if (FILL && row) {
    if (ids_a != nullptr) { at_a = off_a[i]; end_a = off_a[i + 1]; }
    if (ids_b != nullptr) { at_b = off_b[i]; end_b = off_b[i + 1]; }
  }
  int n_a = 0, n_b = 0;

  for (int64_t tile = 0; tile < n_database; tile += RL_TILE) {
    const int len = (int)min((int64_t)RL_TILE, n_database - tile);
    __syncthreads();                                             // the previous tile has been read by every wave
    for (int t = threadIdx.x; t < len; t += RL_THREADS) {
      const int64_t j = tile + t;
      s_db[t] = make_double2(database[2 * j], database[2 * j + 1]);
    }
    __syncthreads();
    if (!row) continue;
    for (int s = 0; s < len; s += HFL_WAVE) {                    // `len` and `s` are uniform: all 64 lanes vote
      const int t = s + lane;
      const bool valid = t < len;
      const double2 p = s_db[valid ? t : 0];
      const double dx = __dsub_rn(qx, p.x), dy = __dsub_rn(qy, p.y);
      const double d2 = __dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy));
      const int64_t j = tile + t;                                // < 2^31: an int32 id
      const bool in_a = valid && d2 <= ra2 && j != self;
      const bool in_b = valid && d2 <= rb2;
      const uint64_t m_a = __ballot(in_a), m_b = __ballot(in_b);
      if (FILL) {
        if (ids_a != nullptr) {
          const int64_t slot = at_a + __popcll(m_a & below);
          if (in_a && slot < end_a) ids_a[slot] = (int32_t)j;
          at_a += __popcll(m_a);
        }
        if (ids_b != nullptr) {
          const int64_t slot = at_b + __popcll(m_b & below);
          if (in_b && slot < end_b) ids_b[slot] = (int32_t)j;
          at_b += __popcll(m_b);
        }
      } else {
        n_a += __popcll(m_a);
        n_b += __popcll(m_b);
      }
    }
  }
  if (!FILL && row && lane < 2) counts[2 * i + lane] = lane == 0 ? n_a : n_b;
}

}  // namespace

extern "C" int hfl_radius_lists(int32_t* counts, int32_t* ids_a, int32_t* ids_b, const int64_t* off_a, const int64_t* off_b,
                                const double* queries, int64_t n_queries, const double* database, int64_t n_database,
                                double r_a, double r_b, int exclude_self, hfl_stream_t stream) {
  if (n_queries < 1 || n_database < 1 || n_database > 0x7fffffffLL || queries == nullptr || database == nullptr)
    return HFL_EINVAL;
  if (!(r_a >= 0.0) || !(r_b >= 0.0) || r_a > r_b) return HFL_EINVAL;                 // negative or NaN
  const int64_t blocks = hfl_cdiv(n_queries, RL_ROWS);
  if (blocks > 0x7fffffffLL) return HFL_EINVAL;
  const bool fill = ids_a != nullptr || ids_b != nullptr;
  if (fill ? ((ids_a != nullptr && off_a == nullptr) || (ids_b != nullptr && off_b == nullptr)) : counts == nullptr)
    return HFL_EINVAL;
  const double ra2 = r_a * r_a, rb2 = r_b * r_b;                 // one multiplication each: nothing to contract
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (fill)
    radius_lists_kernel<true><<<(unsigned)blocks, RL_THREADS, 0, s>>>(counts, ids_a, ids_b, off_a, off_b, queries, n_queries,
                                                                      database, n_database, ra2, rb2, exclude_self);
  else
    radius_lists_kernel<false><<<(unsigned)blocks, RL_THREADS, 0, s>>>(counts, nullptr, nullptr, nullptr, nullptr, queries,
                                                                       n_queries, database, n_database, ra2, rb2,
                                                                       exclude_self);
  HFL_RETURN_LAST_ERROR();
}
