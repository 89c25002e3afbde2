// Compression of the FedAvg uplink with error feedback: the client's update u = (w_k - g) + e against the round's
// starting weights, cut into blocks of 256 coordinates, and what of it did not travel kept in a per-client residual e'
// (Seide et al. 2014; Karimireddy, Rebjock, Stich, Jaggi, ICML 2019).  Two codecs share one encode and one decode
// kernel body and one set of argument checks:
//   * Int8: one fp32 scale per block, 8-bit codes rounded to nearest or stochastically (QSGD: Alistarh, Grubic, Li,
//     Tomioka, Vojnovic, NeurIPS 2017);
//   * TopK: the k coordinates of largest magnitude of every block as (uint8 index, fp32 value), the others whole in
//     the residual (Aji & Heafield, EMNLP 2017; Stich, Cordonnier, Jaggi, NeurIPS 2018).
// The encoder writes the wire chunks of the exchange's send image itself; the decoder rebuilds the fp32 image the
// reduce kernels of optim.hip read.  The contract is in include/mapfed.h.
//
// Every fp32 operation below is rounded on its own (no fused multiply-add), no float atomics, and every store is a
// plain vector store.
#include <stdio.h>
#include "mf_common.h"
#include "philox.h"

#pragma clang fp contract(off)

namespace {

constexpr int QB = 256;  // coordinates per block: one wave64, four per lane

// coordinate i of [fp16 buffer | fp32 buffer], 0 at and past n
MF_DEV float coord(const f16* __restrict__ a16, const float* __restrict__ a32, int64_t n16, int64_t n, int64_t i) {
  return i < n16 ? (float)a16[i] : (i < n ? a32[i - n16] : 0.f);
}

// coordinates i0 .. i0 + 3: one 8-byte load inside the fp16 buffer, one 16-byte load inside the fp32 buffer, where the
// address allows it; element loads across the boundary, past n and at any other address
MF_DEV void load4(const f16* __restrict__ a16, const float* __restrict__ a32, int64_t n16, int64_t n, int64_t i0,
                  float (&v)[4]) {
  if (i0 + 4 <= n16 && ((uintptr_t)(a16 + i0) & 7) == 0) {
    const f16x4 h = *(const f16x4*)(a16 + i0);
#pragma unroll
    for (int l = 0; l < 4; ++l) v[l] = (float)h[l];
  } else if (i0 >= n16 && i0 + 4 <= n && ((uintptr_t)(a32 + (i0 - n16)) & 15) == 0) {
    const f32x4 f = *(const f32x4*)(a32 + (i0 - n16));
#pragma unroll
    for (int l = 0; l < 4; ++l) v[l] = f[l];
  } else {
#pragma unroll
    for (int l = 0; l < 4; ++l) v[l] = coord(a16, a32, n16, n, i0 + l);
  }
}

// the first `left` (all four when left >= 4, none when left <= 0) of the fp32 values at p: one 16-byte access where
// all four are there and the address allows it, element accesses otherwise.  A value that is not loaded stays.
MF_DEV void load4(const float* __restrict__ p, int64_t left, float (&v)[4]) {
  if (left >= 4 && ((uintptr_t)p & 15) == 0) {
    const f32x4 f = *(const f32x4*)p;
#pragma unroll
    for (int l = 0; l < 4; ++l) v[l] = f[l];
  } else {
#pragma unroll
    for (int l = 0; l < 4; ++l)
      if (l < left) v[l] = p[l];
  }
}
MF_DEV void store4(float* __restrict__ p, int64_t left, const float (&v)[4]) {
  if (left >= 4 && ((uintptr_t)p & 15) == 0) {
    f32x4 f;
#pragma unroll
    for (int l = 0; l < 4; ++l) f[l] = v[l];
    *(f32x4*)p = f;
  } else {
#pragma unroll
    for (int l = 0; l < 4; ++l)
      if (l < left) p[l] = v[l];
  }
}

// ---- the codecs.  Each is a kernel argument that knows its part of a wire chunk, the payload ahead of the {weight,
// vote} tail: payload_bytes(nb) for a shard of nb blocks; encode(), one wave for block bj of the chunk, lane l with the
// update u of the block's coordinates 4 l .. 4 l + 3, writes the block's payload and, unless the client is invalid
// (bad: an all-zero payload), leaves in en what of u did not travel; fetch(), the same wave on the receiving side,
// returns in s what travelled of those coordinates when the chunk was sent, and leaves s alone otherwise.  ROBUST:
// whether the decode knows the robust layout.

// [S int8 codes | nb fp32 scales]
struct Int8 {
  static constexpr bool ROBUST = true;
  int stochastic;
  uint32_t k0, k1, round, cword;  // the Philox key, and the counter's upper words

  __host__ __device__ int64_t payload_bytes(int64_t nb) const { return nb * QB + 4 * nb; }

  // blk: the block's index in the whole update; lane l draws the Philox counter 64 * blk + l
  MF_DEV void encode(uint8_t* chunk, int64_t nb, int64_t bj, int64_t blk, int lane, bool bad, const float (&u)[4],
                     float (&en)[4]) const {
    float q[4] = {0.f, 0.f, 0.f, 0.f}, scale = 0.f;
    if (!bad) {
      float amax = 0.f;
#pragma unroll
      for (int l = 0; l < 4; ++l) amax = fmaxf(amax, fabsf(u[l]));
      amax = wave_max(amax);
      scale = amax / 127.0f;
      if (amax == 0.f) {
#pragma unroll
        for (int l = 0; l < 4; ++l) en[l] = u[l];
      } else {
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        if (stochastic) {
          const uint64_t ctr = (uint64_t)blk * 64 + lane;
          philox4x32_10((uint32_t)ctr, (uint32_t)(ctr >> 32), round, cword, k0, k1, w);
        }
#pragma unroll
        for (int l = 0; l < 4; ++l) {
          const float t = u[l] / scale;
          float qq;
          if (stochastic) {
            const float f = floorf(t);
            const float p = t - f;
            const float rr = (float)(w[l] >> 8) * 0x1p-24f;
            qq = f + (rr < p ? 1.f : 0.f);
          } else {
            qq = rintf(t);
          }
          qq = fminf(fmaxf(qq, -127.f), 127.f);  // finite from here on, whatever t was
          q[l] = qq;
          const float sq = scale * qq;
          en[l] = u[l] - sq;
        }
      }
    }
    uint32_t packed = 0u;
#pragma unroll
    for (int l = 0; l < 4; ++l) packed |= ((uint32_t)(int)q[l] & 0xffu) << (8 * l);
    *(uint32_t*)(chunk + bj * QB + 4 * lane) = packed;
    if (lane == 0) *(float*)(chunk + nb * QB + 4 * bj) = scale;
  }

  MF_DEV void fetch(const uint8_t* chunk, int64_t nb, int64_t bj, int lane, bool sent, float (&s)[4]) const {
    if (!sent) return;
    const uint32_t codes = *(const uint32_t*)(chunk + bj * QB + 4 * lane);
    const float scale = *(const float*)(chunk + nb * QB + 4 * bj);
#pragma unroll
    for (int l = 0; l < 4; ++l) s[l] = scale * (float)(int)(int8_t)(codes >> (8 * l));
  }
};

// [nb * k fp32 values | nb * k uint8 indices | zero bytes to a multiple of 4], block bj's entries at bj * k .. + k - 1
// of either region
struct TopK {
  static constexpr bool ROBUST = false;
  int k;

  __host__ __device__ int64_t payload_bytes(int64_t nb) const { return 4 * nb * k + (nb * k + 3) / 4 * 4; }

  // The key of a coordinate is (|u| bits << 8) | (255 - index in the block): 39 bits, distinct within the block, so the
  // k largest keys are the k largest magnitudes with ties going to the lower index.  The k-th largest key is found most
  // significant bit first: a bit stays set when at least k keys reach the candidate, each count four ballots and their
  // popcounts, 39 steps whatever k.  The output position of a kept coordinate is the number of kept coordinates before
  // it.
  MF_DEV void encode(uint8_t* chunk, int64_t nb, int64_t bj, int64_t, int lane, bool bad, const float (&u)[4],
                     float (&en)[4]) const {
    float* vals = (float*)chunk + bj * k;
    uint8_t* idx = chunk + 4 * nb * k + bj * k;
    if (bad) {  // k zero entries
      if (lane < k) {
        vals[lane] = 0.f;
        idx[lane] = 0;
      }
    } else {
      uint64_t key[4];
#pragma unroll
      for (int l = 0; l < 4; ++l)
        key[l] = ((uint64_t)(__float_as_uint(u[l]) & 0x7fffffffu) << 8) | (uint32_t)(255 - (4 * lane + l));
      uint64_t kth = 0;  // wave-uniform
      for (int b = 38; b >= 0; --b) {
        const uint64_t cand = kth | (1ull << b);
        int c = 0;
#pragma unroll
        for (int l = 0; l < 4; ++l) c += __popcll(__ballot(key[l] >= cand));
        if (c >= k) kth = cand;
      }
      bool kept[4];
      int pos = 0;  // kept coordinates of the lower lanes
#pragma unroll
      for (int l = 0; l < 4; ++l) {
        kept[l] = key[l] >= kth;
        const uint64_t m = __ballot(kept[l]);
        pos += __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
      }
#pragma unroll
      for (int l = 0; l < 4; ++l) {
        en[l] = kept[l] ? 0.f : u[l];
        if (kept[l]) {
          vals[pos] = u[l];
          idx[pos] = (uint8_t)(4 * lane + l);
          ++pos;
        }
      }
    }
    if (lane == 0 && bj == nb - 1)  // the index region's padding
      for (int64_t p = 5 * nb * k; p < payload_bytes(nb); ++p) chunk[p] = 0;
  }

  // The wave clears its 1 KB tile of LDS, the lanes below k scatter their entry into it (the index is a byte: it cannot
  // leave the tile), and every lane reads back its four coordinates.  Every wave of the workgroup reaches the barriers.
  MF_DEV void fetch(const uint8_t* chunk, int64_t nb, int64_t bj, int lane, bool sent, float (&s)[4]) const {
    __shared__ __attribute__((aligned(16))) float tile[4][QB];
    float* mine = tile[threadIdx.x >> 6];
    *(f32x4*)&mine[4 * lane] = f32x4{0.f, 0.f, 0.f, 0.f};
    __syncthreads();
    if (sent && lane < k) mine[chunk[4 * nb * k + bj * k + lane]] = ((const float*)chunk)[bj * k + lane];
    __syncthreads();
    if (!sent) return;
    const f32x4 sv = *(const f32x4*)&mine[4 * lane];
#pragma unroll
    for (int l = 0; l < 4; ++l) s[l] = sv[l];
  }
};

// ---- the two kernel bodies

// One wave per block, lane l its coordinates 256 * blk + 4 * l .. + 3.  S is a multiple of 256, so a block lies in one
// destination rank's chunk.  u = (x - g) + e, or x - g without a residual; an invalid client (the flag) sends an
// all-zero payload and the tail {0, 0}, reads no weight and carries its residual over, e' = e.
template <class CODEC>
__global__ __launch_bounds__(256) void encode_kernel(
    const f16* __restrict__ x16, const f16* __restrict__ g16, int64_t n16, const float* __restrict__ x32,
    const float* __restrict__ g32, int64_t n, const float* __restrict__ e_in, float* __restrict__ e_out,
    const int* __restrict__ invalid_flag, float weight, CODEC codec, uint8_t* __restrict__ image, int64_t rank_stride,
    int64_t S, int64_t nblocks) {
  const int lane = threadIdx.x & 63;
  const int64_t blk = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (blk >= nblocks) return;  // the whole wave
  const int64_t i0 = blk * QB + 4 * lane;
  const int64_t nb = S / QB, r = blk / nb, bj = blk - r * nb;
  uint8_t* chunk = image + r * rank_stride;
  const bool bad = invalid_flag != nullptr && *invalid_flag != 0;

  float ev[4] = {0.f, 0.f, 0.f, 0.f}, u[4] = {0.f, 0.f, 0.f, 0.f}, en[4];
  if (e_in) load4(e_in + i0, n - i0, ev);
#pragma unroll
  for (int l = 0; l < 4; ++l) en[l] = ev[l];
  if (!bad) {
    float xv[4], gv[4];
    load4(x16, x32, n16, n, i0, xv);
    load4(g16, g32, n16, n, i0, gv);
#pragma unroll
    for (int l = 0; l < 4; ++l) {
      const float d = xv[l] - gv[l];
      u[l] = e_in ? d + ev[l] : d;
    }
  }
  codec.encode(chunk, nb, bj, blk, lane, bad, u, en);
  if (lane == 0 && bj == 0) {  // the tail, in every destination rank's chunk
    float* tail = (float*)(chunk + codec.payload_bytes(nb));
    tail[0] = bad ? 0.f : weight;
    tail[1] = bad ? 0.f : 1.f;
  }
  if (e_out) store4(e_out + i0, n - i0, en);
}

// blockIdx.y: the chunk (client); one wave per block of its shard, lane l the coordinates j0 .. j0 + 3 of the shard,
// the global coordinates first + c * first_step + j.  y = g + s, s what travelled; out receives w * y (layout 1) or y
// below n, the vote (layout 0) or the weight at n, the vote at n + 1 (layouts 1 and 2) and +0 beyond.  A chunk with
// vote 0, an invalid client's, decodes to what the pack kernels write for it: quiet NaNs in the robust layout (2), a
// codec that has it, and +0 otherwise.
template <class CODEC>
__global__ __launch_bounds__(256) void decode_kernel(const uint8_t* __restrict__ image, int64_t chunk_stride, int64_t S,
                                                     int64_t first, int64_t first_step, const f16* __restrict__ g16,
                                                     int64_t n16, const float* __restrict__ g32, int64_t n, int layout,
                                                     CODEC codec, float* __restrict__ out, int64_t out_stride) {
  const int lane = threadIdx.x & 63;
  const int64_t nb = S / QB, bj = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const bool live = bj < nb;  // per wave
  const int64_t c = blockIdx.y;
  const uint8_t* chunk = image + c * chunk_stride;
  const float* tail = (const float*)(chunk + codec.payload_bytes(nb));
  const float w = tail[0], vote = tail[1];  // uniform over the workgroup
  const bool sent = live && vote != 0.f;
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  codec.fetch(chunk, nb, bj, lane, sent, s);
  if (!live) return;
  const int64_t j0 = bj * QB + 4 * lane, i0 = first + c * first_step + j0;
  float y[4];
  if (sent) {
    float gv[4];
    load4(g16, g32, n16, n, i0, gv);
#pragma unroll
    for (int l = 0; l < 4; ++l) {
      const int64_t i = i0 + l;
      if (i < n) {
        const float yy = gv[l] + s[l];
        y[l] = layout == 1 ? w * yy : yy;
      } else if (i == n) {
        y[l] = layout == 0 ? vote : w;
      } else if (i == n + 1 && layout != 0) {
        y[l] = vote;
      } else {
        y[l] = 0.f;
      }
    }
  } else {
    const float fill = CODEC::ROBUST && layout == 2 ? __uint_as_float(0x7fc00000u) : 0.f;
#pragma unroll
    for (int l = 0; l < 4; ++l) y[l] = fill;
  }
  store4(out + c * out_stride + j0, 4, y);
}

// ---- the entry points' argument checks and launches, the messages under the entry point's name

int fail(const char* name, const char* what) {
  char msg[160];
  snprintf(msg, sizeof(msg), "%s: %s", name, what);
  return mf_set_error(msg, -1);
}

bool shard_ok(int64_t S) { return S > 0 && S % QB == 0; }

// The codec's own arguments are checked by its entry point, ahead of these.
template <class CODEC>
int encode(const char* name, CODEC codec, const void* x16, const void* g16, int64_t n16, const float* x32,
           const float* g32, int64_t n32, const float* e_in, float* e_out, const int* invalid_flag, float weight,
           void* image, int64_t rank_stride, int64_t S, int world, void* stream) {
  if (n16 < 0 || n32 < 0) return fail(name, "negative size");
  if (!shard_ok(S)) return fail(name, "S not a positive multiple of 256");
  if (world < 1) return fail(name, "world < 1");
  if (S > INT64_MAX / world || n16 > INT64_MAX - n32 || n16 + n32 > (int64_t)world * S)
    return fail(name, "world * S shorter than n16 + n32");
  if (!(weight > 0.f) || __builtin_isinf(weight)) return fail(name, "weight not finite and > 0");
  if (!image || !invalid_flag) return fail(name, "null image or flag");
  if ((n16 > 0 && (!x16 || !g16)) || (n32 > 0 && (!x32 || !g32))) return fail(name, "null weights or global copy");
  if ((e_in == nullptr) != (e_out == nullptr) || (e_in && e_in == e_out))
    return fail(name, "residual in and out: both or neither, and two buffers");
  const int64_t chunk = codec.payload_bytes(S / QB) + 8;
  if ((uintptr_t)image % 4 != 0 || rank_stride % 4 != 0 || (world > 1 && rank_stride < chunk))
    return fail(name, "image or rank stride misaligned, or stride below a chunk");
  const int64_t nblocks = (int64_t)world * (S / QB);
  if ((nblocks + 3) / 4 > 0x7fffffff) return fail(name, "too large for one launch");
  encode_kernel<CODEC><<<(unsigned)((nblocks + 3) / 4), 256, 0, (hipStream_t)stream>>>(
      (const f16*)x16, (const f16*)g16, n16, x32, g32, n16 + n32, e_in, e_out, invalid_flag, weight, codec,
      (uint8_t*)image, rank_stride, S, nblocks);
  MF_CHECK_LAUNCH();
  return 0;
}

template <class CODEC>
int decode(const char* name, CODEC codec, const void* image, int64_t chunk_stride, int nclients, int64_t S,
           int64_t first, int64_t first_step, const void* g16, int64_t n16, const float* g32, int64_t n32, int layout,
           float* out, int64_t out_stride, void* stream) {
  if (n16 < 0 || n32 < 0 || first < 0 || first_step < 0) return fail(name, "negative size, first or first_step");
  if (!shard_ok(S)) return fail(name, "S not a positive multiple of 256");
  if (nclients < 1 || nclients > 65535) return fail(name, "nclients outside 1..65535");
  if (layout < 0 || layout > (CODEC::ROBUST ? 2 : 1))
    return fail(name, CODEC::ROBUST ? "unknown layout" : "unknown layout (plain and weighted only)");
  if (!image || !out) return fail(name, "null image or out");
  if ((n16 > 0 && !g16) || (n32 > 0 && !g32)) return fail(name, "null global copy");
  const int64_t chunk = codec.payload_bytes(S / QB) + 8;
  if ((uintptr_t)image % 4 != 0 || chunk_stride % 4 != 0 || (nclients > 1 && (chunk_stride < chunk || out_stride < S)))
    return fail(name, "image or stride misaligned, or a stride below its element");
  if ((uintptr_t)out % 4 != 0) return fail(name, "out not 4-byte aligned");
  if (n16 > INT64_MAX - n32 || first_step > (INT64_MAX - first - S) / nclients)
    return fail(name, "coordinates overflow");
  const int64_t bx = (S / QB + 3) / 4;
  if (bx > 0x7fffffff) return fail(name, "S too large for one launch");
  decode_kernel<CODEC><<<dim3((unsigned)bx, (unsigned)nclients), 256, 0, (hipStream_t)stream>>>(
      (const uint8_t*)image, chunk_stride, S, first, first_step, (const f16*)g16, n16, g32, n16 + n32, layout, codec,
      out, out_stride);
  MF_CHECK_LAUNCH();
  return 0;
}

bool topk_ok(int k) { return k >= 1 && k <= 64; }

}  // namespace

// bytes of one wire chunk of shard length S: the codec's payload, then [fp32 weight | fp32 vote]
extern "C" int64_t mf_compress_chunk_bytes(int64_t S) { return shard_ok(S) ? Int8{}.payload_bytes(S / QB) + 8 : -1; }

extern "C" int64_t mf_topk_chunk_bytes(int64_t S, int k) {
  return shard_ok(S) && topk_ok(k) ? TopK{k}.payload_bytes(S / QB) + 8 : -1;
}

extern "C" int mf_compress_quantize(const void* x16, const void* g16, int64_t n16, const float* x32, const float* g32,
                                    int64_t n32, const float* e_in, float* e_out, const int* invalid_flag,
                                    float weight, int rounding, uint64_t seed, uint32_t round, uint32_t client,
                                    void* image, int64_t rank_stride, int64_t S, int world, void* stream) {
  const char* name = "mf_compress_quantize";
  if (rounding != 0 && rounding != 1) return fail(name, "unknown rounding");
  if (client >= 0x80000000u) return fail(name, "client index above 2^31 - 1");
  return encode(name, Int8{rounding, (uint32_t)seed, (uint32_t)(seed >> 32), round, 0x80000000u | client}, x16, g16,
                n16, x32, g32, n32, e_in, e_out, invalid_flag, weight, image, rank_stride, S, world, stream);
}

extern "C" int mf_compress_decode(const void* image, int64_t chunk_stride, int nclients, int64_t S, int64_t first,
                                  int64_t first_step, const void* g16, int64_t n16, const float* g32, int64_t n32,
                                  int layout, float* out, int64_t out_stride, void* stream) {
  return decode("mf_compress_decode", Int8{}, image, chunk_stride, nclients, S, first, first_step, g16, n16, g32, n32,
                layout, out, out_stride, stream);
}

extern "C" int mf_topk_select(const void* x16, const void* g16, int64_t n16, const float* x32, const float* g32,
                              int64_t n32, const float* e_in, float* e_out, const int* invalid_flag, float weight, int k,
                              void* image, int64_t rank_stride, int64_t S, int world, void* stream) {
  const char* name = "mf_topk_select";
  if (!topk_ok(k)) return fail(name, "k outside 1..64");
  return encode(name, TopK{k}, x16, g16, n16, x32, g32, n32, e_in, e_out, invalid_flag, weight, image, rank_stride, S,
                world, stream);
}

extern "C" int mf_topk_decode(const void* image, int64_t chunk_stride, int nclients, int64_t S, int64_t first,
                              int64_t first_step, const void* g16, int64_t n16, const float* g32, int64_t n32, int layout,
                              float* out, int64_t out_stride, int k, void* stream) {
  const char* name = "mf_topk_decode";
  if (!topk_ok(k)) return fail(name, "k outside 1..64");
  return decode(name, TopK{k}, image, chunk_stride, nclients, S, first, first_step, g16, n16, g32, n32, layout, out,
                out_stride, stream);
}
