// Multi-Krum (Blanchard, El Mhamdi, Guerraoui, Stainer: "Machine Learning with Adversaries: Byzantine Tolerant
// Gradient Descent", NeurIPS 2017; the "keep the m best" form of El Mhamdi, Guerraoui, Rouault, ICML 2018) over the
// [client][coordinate] image reduce_ordered_kernel sums: the pairwise squared L2 distances of the clients, the
// selection of whole clients by their distances to their nearest peers, and the mean of the selected clients.  The
// contract of all three is in include/mapfed.h.
//
// The distances are differences first, never a Gram matrix: the clients all start from the same global weights, so
// G_ii + G_jj - 2 G_ij would cancel.  No float atomics; every sum below has a fixed order.
#include "mf_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int CHUNK = 8192;                  // coordinates per workgroup of the first launch
constexpr int TILE = 8;                      // clients per side of a pair tile: 64 fp64 accumulators per thread
constexpr int GROUPS = CHUNK / (4 * 256);    // groups of 4 coordinates per thread and chunk
constexpr int FINISH_WAVES = 16;             // runs of chunks the second launch sums side by side
constexpr unsigned long long QNAN64 = 0x7ff8000000000000ull;

inline unsigned nblk(int64_t n, int b = 256) { return (unsigned)((n + b - 1) / b); }
inline bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p % a) == 0; }
inline int64_t nchunks(int64_t n) { return (n + CHUNK - 1) / CHUNK; }
inline int ntiles(int nclients) { return (nclients + TILE - 1) / TILE; }
inline int npairs(int nclients) { return ntiles(nclients) * (ntiles(nclients) + 1) / 2; }

// pair index -> (ti, tj), ti <= tj, in the order (0,0) (0,1) .. (0,T-1) (1,1) ..
MF_DEV void pair_tiles(int pair, int nt, int& ti, int& tj) {
  ti = 0;
  while (pair >= nt - ti) {
    pair -= nt - ti;
    ++ti;
  }
  tj = ti + pair;
}

// One butterfly level of the wave reduction of 64 accumulators: the lanes l and l ^ H add their values of one half of
// the remaining 2H accumulators each, so 63 exchanges reduce all 64 (a plain butterfly takes 384) and lane l ends
// with the wave's sum of accumulator l.  The tree is the xor butterfly's: 32, 16, .., 1, the same on every launch.
template <int H>
MF_DEV void fold(double (&acc)[TILE * TILE], int lane) {
  const bool up = (lane & H) != 0;
#pragma unroll
  for (int k = 0; k < H; ++k) {
    const double send = up ? acc[k] : acc[k + H];
    const double keep = up ? acc[k + H] : acc[k];
    acc[k] = keep + __shfl_xor(send, H, 64);
  }
}

// Block (chunk, pair): the 8 x 8 partial distances of client tiles (ti, tj) over the chunk's coordinates.  Thread t
// owns the groups of 4 coordinates t, t + 256, ... of the chunk and adds them in ascending order, whatever the load
// width: VEC takes one 16-byte load per client where the whole group lies below n, 4-byte loads otherwise; a
// coordinate at or past n adds +0.  A row past nclients re-reads the last client (its entries are never written out).
// A tile of a pair with itself (DIAG) loads its 8 clients once and forms the 36 pairs a <= b only; the other
// accumulators stay +0 and are never written out.
template <bool VEC>
MF_DEV void load_tile(const float* const (&r)[TILE], int64_t i, int64_t n, f32x4 (&x)[TILE]) {
  if (VEC && i + 4 <= n) {
#pragma unroll
    for (int a = 0; a < TILE; ++a) x[a] = *(const f32x4*)(r[a] + i);
  } else {
#pragma unroll
    for (int a = 0; a < TILE; ++a)
#pragma unroll
      for (int e = 0; e < 4; ++e) x[a][e] = i + e < n ? r[a][i + e] : 0.f;
  }
}

template <bool VEC, bool DIAG>
MF_DEV void chunk_pairs(const float* const (&ri)[TILE], const float* const (&rj)[TILE], int64_t c0, int64_t n,
                        double (&acc)[TILE * TILE]) {
  for (int k = 0; k < GROUPS; ++k) {
    const int64_t i = c0 + 4 * ((int64_t)threadIdx.x + 256 * k);
    if (i >= n) break;
    f32x4 xi[TILE], xj[TILE];
    load_tile<VEC>(ri, i, n, xi);
    if constexpr (!DIAG) load_tile<VEC>(rj, i, n, xj);
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int a = 0; a < TILE; ++a)
#pragma unroll
        for (int b = DIAG ? a : 0; b < TILE; ++b) {
          const double d = (double)(xi[a][e] - (DIAG ? xi[b][e] : xj[b][e]));
          acc[a * TILE + b] = __builtin_fma(d, d, acc[a * TILE + b]);  // d * d is exact in fp64: mul + add's bits
        }
  }
}

template <bool VEC>
__global__ __launch_bounds__(256) void krum_pair_kernel(const float* __restrict__ g, int nclients, int64_t stride,
                                                        int64_t n, int nt, int np, double* __restrict__ part) {
  const int64_t chunk = blockIdx.x / (unsigned)np;
  int ti, tj;
  pair_tiles((int)(blockIdx.x % (unsigned)np), nt, ti, tj);
  const float* ri[TILE];
  const float* rj[TILE];
#pragma unroll
  for (int a = 0; a < TILE; ++a) {
    ri[a] = g + (int64_t)min(ti * TILE + a, nclients - 1) * stride;
    rj[a] = g + (int64_t)min(tj * TILE + a, nclients - 1) * stride;
  }
  double acc[TILE * TILE];
#pragma unroll
  for (int k = 0; k < TILE * TILE; ++k) acc[k] = 0.0;
  if (ti == tj)
    chunk_pairs<VEC, true>(ri, rj, chunk * CHUNK, n, acc);
  else
    chunk_pairs<VEC, false>(ri, rj, chunk * CHUNK, n, acc);
  const int lane = threadIdx.x & 63;
  fold<32>(acc, lane);
  fold<16>(acc, lane);
  fold<8>(acc, lane);
  fold<4>(acc, lane);
  fold<2>(acc, lane);
  fold<1>(acc, lane);
  __shared__ double red[4][TILE * TILE];
  red[threadIdx.x >> 6][lane] = acc[0];
  __syncthreads();
  if (threadIdx.x < TILE * TILE)
    part[(int64_t)blockIdx.x * (TILE * TILE) + lane] = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
}

// Block per pair tile: the chunk partials in chunk order (wave w sums a contiguous run of chunks, wave 0 the 16 runs
// in order), written to dist[i][j] and mirrored to dist[j][i] for i <= j < nclients.  No chunk: the zero matrix.
__global__ __launch_bounds__(64 * FINISH_WAVES) void krum_finish_kernel(const double* __restrict__ part, int64_t nc,
                                                                        int nclients, int nt, int np,
                                                                        double* __restrict__ dist) {
  __shared__ double red[FINISH_WAVES][TILE * TILE];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t per = (nc + FINISH_WAVES - 1) / FINISH_WAVES;
  const int64_t lo = min(nc, (int64_t)w * per), hi = min(nc, lo + per);
  double s = 0.0;
  for (int64_t c = lo; c < hi; ++c) s += part[(c * np + blockIdx.x) * (TILE * TILE) + lane];
  red[w][lane] = s;
  __syncthreads();
  if (w != 0) return;
  double tot = 0.0;
  for (int k = 0; k < FINISH_WAVES; ++k) tot += red[k][lane];
  int ti, tj;
  pair_tiles((int)blockIdx.x, nt, ti, tj);
  const int i = ti * TILE + (lane >> 3), j = tj * TILE + (lane & 7);
  if (i < nclients && j < nclients && i <= j) {
    dist[(int64_t)i * nclients + j] = tot;
    dist[(int64_t)j * nclients + i] = tot;
  }
}

// the order of the non-negative doubles, +inf and the NaNs above them, as an unsigned compare; with the index, a
// strict total order on (value, client)
MF_DEV bool key_less(unsigned long long va, int ia, unsigned long long vb, int ib) {
  return va < vb || (va == vb && ia < ib);
}

// One workgroup: combine, presence, scores, selection (the contract of include/mapfed.h, step by step)
__global__ __launch_bounds__(256) void krum_select_kernel(const double* __restrict__ parts, int nparts, int nclients,
                                                          int f, int m, int* __restrict__ selected,
                                                          double* __restrict__ scores, int* __restrict__ counts) {
  __shared__ double D[64 * 64];
  __shared__ double score[64];
  __shared__ int present[64];
  const int nn = nclients * nclients;
  for (int e = threadIdx.x; e < nn; e += blockDim.x) {
    double s = parts[e];
    for (int r = 1; r < nparts; ++r) s += parts[(int64_t)r * nn + e];
    D[e] = s;
  }
  __syncthreads();
  if (threadIdx.x < 64) {
    const double d = threadIdx.x < nclients ? D[threadIdx.x * nclients + threadIdx.x] : __longlong_as_double(QNAN64);
    present[threadIdx.x] = d == d;
  }
  __syncthreads();
  int p = 0;
  for (int c = 0; c < nclients; ++c) p += present[c];
  const int fe = max(min(f, p >= 3 ? (p - 3) / 2 : 0), 0);
  const int q = max(p - fe - 2, 0);
  const int me = m == 0 ? p - fe : min(m, p - fe);
  const int i = threadIdx.x;
  if (i < nclients) {
    double sc = __longlong_as_double(QNAN64);
    if (present[i]) {
      // the q smallest D[i][j] over present j != i in ascending (value, j) order: each pass takes the least key
      // above the last one taken
      sc = 0.0;
      unsigned long long lastv = 0;
      int lastj = -1;
      for (int t = 0; t < q; ++t) {
        unsigned long long bestv = ~0ull;
        int bestj = 64;
        for (int j = 0; j < nclients; ++j) {
          if (j == i || !present[j]) continue;
          const unsigned long long v = (unsigned long long)__double_as_longlong(D[i * nclients + j]);
          if (key_less(lastv, lastj, v, j) && key_less(v, j, bestv, bestj)) {
            bestv = v;
            bestj = j;
          }
        }
        const double term = __longlong_as_double((long long)bestv);
        sc = t == 0 ? term : sc + term;
        lastv = bestv;
        lastj = bestj;
      }
    }
    score[i] = sc;
    scores[i] = sc;
  }
  __syncthreads();
  if (i < nclients) {
    int sel = 0;
    if (present[i]) {
      const unsigned long long mine = (unsigned long long)__double_as_longlong(score[i]);
      int rank = 0;
      for (int j = 0; j < nclients; ++j)
        if (present[j] && key_less((unsigned long long)__double_as_longlong(score[j]), j, mine, i)) ++rank;
      sel = rank < me;
    }
    selected[i] = sel;
  }
  if (i == 0) {
    counts[0] = p;
    counts[1] = fe;
    counts[2] = me;
  }
}

// Each thread owns VEC whole coordinates i .. i + VEC - 1 < n (the launcher sees to that), as in
// reduce_trimmed_kernel: the selected clients' values in client order, the first one taken as it is and one fp32 add
// for each further one -- an unselected client is never loaded, let alone multiplied by 0 -- divided by their number;
// at count_pos the number of non-NaN values over all the clients instead.
template <int VEC>
__global__ __launch_bounds__(256) void reduce_selected_kernel(const float* __restrict__ g, int nclients,
                                                              int64_t stride, int64_t n,
                                                              const int* __restrict__ selected, int64_t count_pos,
                                                              float* __restrict__ out) {
  __shared__ unsigned long long smask;
  if (threadIdx.x < 64) {
    const unsigned long long b = __ballot(threadIdx.x < nclients && selected[min((int)threadIdx.x, nclients - 1)] != 0);
    if (threadIdx.x == 0) smask = b;
  }
  __syncthreads();
  const unsigned long long mask = smask;
  const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * VEC;
  if (i >= n) return;
  const float m = (float)__popcll(mask);
  float r[VEC];
#pragma unroll
  for (int e = 0; e < VEC; ++e) r[e] = 0.f;
  if (mask != 0) {
    unsigned long long rest = mask;
    int c = __ffsll((long long)rest) - 1;
    rest &= rest - 1;
    if constexpr (VEC == 4) {
      f32x4 acc = *(const f32x4*)(g + (int64_t)c * stride + i);
      for (; rest != 0; rest &= rest - 1) {
        c = __ffsll((long long)rest) - 1;
        const f32x4 v = *(const f32x4*)(g + (int64_t)c * stride + i);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = acc[e] + v[e];
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) r[e] = acc[e] / m;
    } else {
      float acc = g[(int64_t)c * stride + i];
      for (; rest != 0; rest &= rest - 1) {
        c = __ffsll((long long)rest) - 1;
        acc = acc + g[(int64_t)c * stride + i];
      }
      r[0] = acc / m;
    }
  }
  if (count_pos >= i && count_pos < i + VEC) {
    int p = 0;
    for (int c = 0; c < nclients; ++c) {
      const float v = g[(int64_t)c * stride + count_pos];
      p += v == v;
    }
#pragma unroll
    for (int e = 0; e < VEC; ++e)
      if (count_pos == i + e) r[e] = (float)p;
  }
  if constexpr (VEC == 4) {
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = r[e];
    *(f32x4*)(out + i) = o;
  } else {
    out[i] = r[0];
  }
}

}  // namespace

extern "C" int mf_krum_chunk_elems(void) { return CHUNK; }

// bytes of workspace mf_krum_pairwise needs: one 8 x 8 fp64 tile per chunk and pair of client tiles (at least one)
extern "C" int64_t mf_krum_ws_bytes(int nclients, int64_t n) {
  if (nclients < 1 || nclients > 64 || n < 0) return -1;
  const int64_t tiles = nchunks(n) * npairs(nclients);
  return (tiles > 0 ? tiles : 1) * (int64_t)(TILE * TILE * sizeof(double));
}

extern "C" int mf_krum_pairwise(const float* gathered, int nclients, int64_t stride, int64_t n, void* ws, double* dist,
                                void* stream) {
  if (nclients < 1 || nclients > 64) return mf_set_error("mf_krum_pairwise: nclients not in [1, 64]", -1);
  if (n < 0 || stride < n) return mf_set_error("mf_krum_pairwise: bad sizes (n < 0 or stride < n)", -1);
  if (!ws || !dist) return mf_set_error("mf_krum_pairwise: null workspace or dist", -1);
  if (!aligned(ws, 8) || !aligned(dist, 8)) return mf_set_error("mf_krum_pairwise: ws / dist not 8-byte aligned", -1);
  if (n > 0 && !gathered) return mf_set_error("mf_krum_pairwise: null gathered", -1);
  if (n > 0 && !aligned(gathered, 4)) return mf_set_error("mf_krum_pairwise: gathered not 4-byte aligned", -1);
  const int nt = ntiles(nclients), np = npairs(nclients);
  const int64_t nc = nchunks(n);
  if (nc * np > 0x7fffffff) return mf_set_error("mf_krum_pairwise: too many chunks for one launch", -1);
  hipStream_t st = (hipStream_t)stream;
  if (nc > 0) {
    if (stride % 4 == 0 && aligned(gathered, 16))
      krum_pair_kernel<true><<<(unsigned)(nc * np), 256, 0, st>>>(gathered, nclients, stride, n, nt, np, (double*)ws);
    else
      krum_pair_kernel<false><<<(unsigned)(nc * np), 256, 0, st>>>(gathered, nclients, stride, n, nt, np, (double*)ws);
    MF_CHECK_LAUNCH();
  }
  krum_finish_kernel<<<(unsigned)np, 64 * FINISH_WAVES, 0, st>>>((const double*)ws, nc, nclients, nt, np, dist);
  MF_CHECK_LAUNCH();
  return 0;
}

extern "C" int mf_krum_select(const double* parts, int nparts, int nclients, int f, int m, int* selected,
                              double* scores, int* counts, void* stream) {
  if (nparts < 1) return mf_set_error("mf_krum_select: nparts < 1", -1);
  if (nclients < 1 || nclients > 64) return mf_set_error("mf_krum_select: nclients not in [1, 64]", -1);
  if (f < 0) return mf_set_error("mf_krum_select: f < 0", -1);
  if (m < 0) return mf_set_error("mf_krum_select: m < 0", -1);
  if (!parts || !selected || !scores || !counts) return mf_set_error("mf_krum_select: null pointer", -1);
  krum_select_kernel<<<1, 256, 0, (hipStream_t)stream>>>(parts, nparts, nclients, f, m, selected, scores, counts);
  MF_CHECK_LAUNCH();
  return 0;
}

// Multi-Krum's reduce in mf_fedavg_reduce_trimmed's place (same image): the mean of the selected clients
extern "C" int mf_fedavg_reduce_selected(const float* gathered, int nclients, int64_t stride, int64_t n,
                                         const int* selected, int64_t count_pos, float* out, void* stream) {
  if (nclients < 1 || nclients > 64) return mf_set_error("mf_fedavg_reduce_selected: nclients not in [1, 64]", -1);
  if (n < 0 || stride < n) return mf_set_error("mf_fedavg_reduce_selected: bad sizes (n < 0 or stride < n)", -1);
  if (count_pos >= n) return mf_set_error("mf_fedavg_reduce_selected: count_pos >= n", -1);
  if (n == 0) return 0;
  if (!gathered || !out || !selected) return mf_set_error("mf_fedavg_reduce_selected: null pointer", -1);
  hipStream_t st = (hipStream_t)stream;
  int64_t n4 = 0;
  if (stride % 4 == 0 && aligned(gathered, 16) && aligned(out, 16)) n4 = n & ~(int64_t)3;
  if (n4 > 0)
    reduce_selected_kernel<4><<<nblk(n4 / 4), 256, 0, st>>>(gathered, nclients, stride, n4, selected, count_pos, out);
  if (n > n4)
    reduce_selected_kernel<1><<<nblk(n - n4), 256, 0, st>>>(gathered + n4, nclients, stride, n - n4, selected,
                                                            count_pos - n4, out + n4);
  MF_CHECK_LAUNCH();
  return 0;
}
