// kmg_gkm.hip — the gapped k-mer (gkm) kernel of gkm-SVM / LS-GKM for gfx950.
//
//   K(x, y) = sum_{a, b} h[ham(x[a:a+l], y[b:b+l])],  h[m] = C(l - m, k) for m <= d, else 0
//
// (Ghandi, Lee, Mohammad-Noori, Beer: "Enhanced regulatory sequence prediction using gapped
// k-mer features", PLoS Comput Biol 2014: the number of gapped k-mers -- l-mers with k
// informative positions -- two words at Hamming distance m share, truncated at d mismatches.)
// a and b run over the all-ACGT words of the whole row; every value is an integer, and with at
// most 256 words a row the raw sum stays below 256^2 C(16, 8) < 2^31, so everything up to the
// float epilogue is int32.
//
// Input: the [n][pmax] array of 2-bit words launch_extract writes (KMG_INVALID for a window
// that holds a non-ACGT symbol or runs past the row).  At l = 16 the word T^16 is the same 32
// bits as KMG_INVALID and is dropped, as in every packed k = 16 path of the library.
//
// gram_gkm_kernel: one 256-thread workgroup a tile of 16 x 16 sequences.
//   LDS     the words of the tile's 16 rows and 16 columns, staged once ((16 + 16) * pp words,
//           pp = pmax rounded up to 4: <= 32 KB), the weight table (34 int32: h[0..16], then 17
//           zeros) and the 16 x 17 int32 result tile.
//   waves   wave w owns rows 4w .. 4w + 3 of the tile and walks their 16 columns, one (row,
//           column) pair at a time.
//   lanes   32 row-word slots x 2 column halves.  Lane (slot, half) keeps the row's words slot,
//           slot + 32, ... in NQ = ceil(pmax / 32) registers and walks the column's words in
//           16-byte pieces, half 0 the even pieces, half 1 the odd ones (one ds_read_b128 of two
//           addresses a wave).  At 92 words a row (L = 101, l = 10) the slots are 92 / 96 full;
//           64 slots x one column stream would leave its second stride 28 / 64 full (72 % of the
//           lane slots used over the pair).
//   word    x = xa ^ yb; t = ((x << 1) | x) & maskAA (one bit a differing letter, ham2bit's
//           mask one bit up, so shift and or are one v_lshl_or_b32); idx = popc(t) + base
//           (v_bcnt_u32_b32 adds its second operand); s += w_s[idx].  base is 17 for an invalid
//           or absent row word, which lands in the zero half of the table: no divergence.  An
//           invalid column word zeroes the sum of its NQ lookups with one select (the two
//           halves read different words, so a skip would not be wave-uniform).
//   pair    one xor-shuffle reduction, lane 0 writes the result tile.
//   SYM     (the launch covers all n rows) only tiles with column tile >= row tile are
//           scheduled; an off-diagonal tile also stores its transpose from the LDS result tile,
//           so both stores are row-contiguous; a diagonal tile computes j >= i and mirrors
//           inside LDS.
//   edges   rows past row1 and columns past n are not staged, computed or stored.
//   RC      both strands (kmg_params.strands = 2, l <= 15):
//             K2(x, y) = K(x, y) + K(x, rc(y)),  rc = reverse complement (code c -> c ^ 3)
//           The l-mers of rc(y) are the reverse complements of the l-mers of y, so staging also
//           writes the columns' reverse-complement words into a third LDS array [16][pp]
//           (<= 16 KB more): (pairrev32(w) >> (32 - 2l)) ^ ((1 << 2l) - 1), KMG_INVALID kept.
//           The inner step reads the forward and the reverse-complement 16-byte piece and adds
//           both lookups; the two words are valid together, so the column select is shared.
//           K2 is symmetric (ham(u, rc(v)) = ham(v, rc(u))), so SYM, the mirror and the
//           transposed store are the single-strand ones.  K2 is half the inner product of the
//           strand-symmetrised feature map c(x) + c(rc(x)); the factor 2 cancels under
//           normalisation.  Still int32: 2 * 256^2 C(16, 8) < 2^31.  l = 16 is refused by the
//           caller: rc(A^16) = T^16 is KMG_INVALID's bits, and dropping it on one strand only
//           would break the symmetry SYM relies on.
// gkm_diag_kernel: K_ii for the fused normalize_K, one wave a sequence, four a workgroup.
#include "kmg_internal.h"
#include "kmg_rowacc.h"

namespace kmg {

namespace {

constexpr int GKM_T = 16;        // tile edge (sequences)
constexpr int GKM_RES_LD = 17;   // result tile row stride (transposed reads: distinct banks)
constexpr int GKM_WTAB = 34;     // h[0..16], then 17 zeros

__device__ __forceinline__ uint32_t gkm_mask(int l) {
  return l >= 16 ? 0xAAAAAAAAu : (0xAAAAAAAAu & ((1u << (2 * l)) - 1u));
}
// Hamming distance of two l-letter 2-bit words, plus base
__device__ __forceinline__ int gkm_dist(uint32_t a, uint32_t b, uint32_t maskAA, int base) {
  const uint32_t x = a ^ b;
  return __popc(((x << 1) | x) & maskAA) + base;
}

// reverse complement of an l-letter word (l <= 15), right-aligned like w; KMG_INVALID stays
__device__ __forceinline__ uint32_t gkm_rcword(uint32_t w, int l) {
  const uint32_t r = __builtin_bitreverse32(w);
  const uint32_t pr = ((r & 0x55555555u) << 1) | ((r >> 1) & 0x55555555u);  // pairs reversed
  return w == KMG_INVALID ? KMG_INVALID : (pr >> (32 - 2 * l)) ^ ((1u << (2 * l)) - 1u);
}

__device__ __forceinline__ void gkm_load_weights(const GkmWeights &wt, int32_t *w_s) {
  // constant indices only: the table stays in scalar registers, no scratch copy
#pragma unroll
  for (int d = 0; d < 17; ++d)
    if (threadIdx.x == d) w_s[d] = wt.h[d];
  if (threadIdx.x >= 17 && threadIdx.x < GKM_WTAB) w_s[threadIdx.x] = 0;
}

// first tile index of row tr of the upper block triangle (T tiles a side), row-major
__device__ __forceinline__ int64_t gkm_tri_first(int64_t tr, int64_t T) {
  return tr * T - tr * (tr - 1) / 2;
}

__device__ __forceinline__ void gkm_emit(const OutSpec &o, int64_t il, int64_t ig, int64_t col,
                                         int cnt, const int32_t *v, int stride, bool norm) {
  const int64_t v0 = v[0], v1 = v[stride], v2 = v[2 * stride], v3 = v[3 * stride];
  switch (o.dtype) {
    case KMG_I32: emit4<KMG_I32>(o, il, ig, col, cnt, v0, v1, v2, v3, norm); break;
    case KMG_F32: emit4<KMG_F32>(o, il, ig, col, cnt, v0, v1, v2, v3, norm); break;
    default: emit4<KMG_F64>(o, il, ig, col, cnt, v0, v1, v2, v3, norm); break;
  }
}

template <int NQ, bool SYM, bool RC>
__global__ __launch_bounds__(256) void gram_gkm_kernel(const uint32_t *__restrict__ words, int pmax,
                                                       int l, int64_t n, int64_t row0, int64_t rows,
                                                       int64_t tiles_c, GkmWeights wt, OutSpec o) {
  extern __shared__ __align__(16) uint32_t gkm_lds[];
  const int pp = (pmax + 3) & ~3;
  uint32_t *rw = gkm_lds;                                    // [16][pp] row words
  uint32_t *cwd = gkm_lds + GKM_T * pp;                      // [16][pp] column words
  uint32_t *crc = gkm_lds + 2 * GKM_T * pp;                  // [16][pp] their rc words (RC)
  int32_t *w_s = (int32_t *)(gkm_lds + (RC ? 3 : 2) * GKM_T * pp);  // [GKM_WTAB]
  int32_t *res = w_s + GKM_WTAB + 2;                         // [16][GKM_RES_LD]

  int64_t tr, tc;
  if constexpr (SYM) {
    const int64_t b = blockIdx.x, T = tiles_c;
    const double t2 = 2.0 * (double)T + 1.0;
    tr = (int64_t)((t2 - __builtin_sqrt(t2 * t2 - 8.0 * (double)b)) * 0.5);
    tr = max((int64_t)0, min(tr, T - 1));
    while (tr + 1 < T && gkm_tri_first(tr + 1, T) <= b) ++tr;
    while (tr > 0 && gkm_tri_first(tr, T) > b) --tr;
    tc = tr + (b - gkm_tri_first(tr, T));
  } else {
    tr = (int64_t)blockIdx.x / tiles_c;
    tc = (int64_t)blockIdx.x - tr * tiles_c;
  }
  const int64_t i0 = row0 + tr * GKM_T, j0 = tc * GKM_T;
  const int nr = (int)min((int64_t)GKM_T, row0 + rows - i0);
  const int nc = (int)min((int64_t)GKM_T, n - j0);
  const bool diag_tile = SYM && tr == tc;

  gkm_load_weights(wt, w_s);
  for (int t = threadIdx.x; t < 2 * GKM_T * pp; t += 256) {
    const int s = t / pp, a = t - s * pp;
    const bool row = s < GKM_T;
    const int sl = row ? s : s - GKM_T;
    const bool ok = a < pmax && sl < (row ? nr : nc);
    const uint32_t w = ok ? words[((row ? i0 : j0) + sl) * pmax + a] : KMG_INVALID;
    gkm_lds[t] = w;
    if (RC && !row) crc[sl * pp + a] = gkm_rcword(w, l);
  }
  __syncthreads();

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int slot = lane & 31, half = lane >> 5;
  const uint32_t maskAA = gkm_mask(l);
  for (int rr = 0; rr < GKM_T / 4; ++rr) {
    const int r = wave * (GKM_T / 4) + rr;
    if (r >= nr) break;  // wave-uniform
    uint32_t xa[NQ];
    int base[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int a = slot + 32 * q;
      xa[q] = a < pp ? rw[r * pp + a] : KMG_INVALID;
      base[q] = xa[q] == KMG_INVALID ? 17 : 0;
    }
    for (int c = diag_tile ? r : 0; c < nc; ++c) {
      const uint32_t *cs = cwd + c * pp;
      int s = 0;
      for (int b0 = 4 * half; b0 < pmax; b0 += 8) {
        const uint4 y4 = *(const uint4 *)(cs + b0);
        const uint32_t y[4] = {y4.x, y4.y, y4.z, y4.w};
        uint32_t z[4] = {};
        if constexpr (RC) {
          const uint4 z4 = *(const uint4 *)(crc + c * pp + b0);
          z[0] = z4.x, z[1] = z4.y, z[2] = z4.z, z[3] = z4.w;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          int sw = 0;
#pragma unroll
          for (int q = 0; q < NQ; ++q) {
            sw += w_s[gkm_dist(xa[q], y[e], maskAA, base[q])];
            if constexpr (RC) sw += w_s[gkm_dist(xa[q], z[e], maskAA, base[q])];
          }
          s += y[e] == KMG_INVALID ? 0 : sw;  // z[e] is invalid exactly when y[e] is
        }
      }
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
      if (lane == 0) res[r * GKM_RES_LD + c] = s;
    }
  }
  __syncthreads();
  if (diag_tile) {  // block-uniform
    const int r = threadIdx.x >> 4, c = threadIdx.x & 15;
    if (c < r && r < nr) res[r * GKM_RES_LD + c] = res[c * GKM_RES_LD + r];
    __syncthreads();
  }

  // 64 threads a direction: thread (row, group of 4 columns), 64 contiguous bytes a row at int32
  const bool norm = o.normalize && o.diagv[0] != 1.0;
  const int t = threadIdx.x & 63, r = t >> 2, cg = (t & 3) * 4;
  if (threadIdx.x < 64) {
    if (r < nr && cg < nc)
      gkm_emit(o, i0 - row0 + r, i0 + r, j0 + cg, min(4, nc - cg), res + r * GKM_RES_LD + cg, 1,
               norm);
  } else if (SYM && !diag_tile && threadIdx.x < 128) {
    // the transpose: row j0 + r of K at columns i0 + cg .. (SYM: row0 = 0, so local = global)
    if (r < nc && cg < nr)
      gkm_emit(o, j0 + r, j0 + r, i0 + cg, min(4, nr - cg), res + cg * GKM_RES_LD + r, GKM_RES_LD,
               norm);
  }
}

// K_ii = sum_{a, b} h[ham(x_a, x_b)] is symmetric in (a, b): the b > a half counted twice plus
// the a = b term.  Lane t takes the words a = t and a = P - 1 - t (and so on in strides of
// 128), whose tails add up to ~P iterations for every lane, as diag_ham_small_kernel does.
// RC adds sum_{a, b} h[ham(x_a, rc(x_b))], symmetric in (a, b) as well (ham(u, rc(v)) =
// ham(v, rc(u))): the same tails, with the a = b term h[ham(x_a, rc(x_a))] instead of h[0].
template <bool RC>
__global__ __launch_bounds__(256) void gkm_diag_kernel(const uint32_t *__restrict__ words, int pmax,
                                                       int l, int64_t n, GkmWeights wt,
                                                       double *__restrict__ diagv,
                                                       double *__restrict__ dsq) {
  extern __shared__ __align__(16) uint32_t gkm_lds[];  // [4][pmax] words, then the weights
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + wave;
  const bool valid = i < n;
  const int P = pmax;
  uint32_t *xk = gkm_lds + wave * P;
  int32_t *w_s = (int32_t *)(gkm_lds + 4 * P);
  gkm_load_weights(wt, w_s);
  if (valid)
    for (int a = lane; a < P; a += 64) xk[a] = words[i * P + a];
  __syncthreads();
  if (!valid) return;
  const uint32_t maskAA = gkm_mask(l);
  int s = 0;
  auto tail = [&](int a) {
    const uint32_t xa = xk[a];
    if (xa == KMG_INVALID) return;
    s += w_s[0];  // b = a
    if constexpr (RC) s += w_s[gkm_dist(xa, gkm_rcword(xa, l), maskAA, 0)];
    for (int b = a + 1; b < P; ++b) {
      const uint32_t yb = xk[b];
      const int base = yb == KMG_INVALID ? 17 : 0;
      s += 2 * w_s[gkm_dist(xa, yb, maskAA, base)];
      if constexpr (RC) s += 2 * w_s[gkm_dist(xa, gkm_rcword(yb, l), maskAA, base)];
    }
  };
  for (int a0 = 0; a0 < (P + 1) / 2; a0 += 64) {
    const int a = a0 + lane, a2 = P - 1 - a;
    if (a < (P + 1) / 2) {
      tail(a);
      if (a2 != a) tail(a2);
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
  if (lane == 0) {
    const double v = (double)s;
    diagv[i] = v;
    dsq[i] = __builtin_sqrt(v);  // np.sqrt(np.diag(K)) (kernels.py:408): IEEE sqrt
  }
}

}  // namespace

int64_t gkm_tiles(int64_t n, int64_t rows, bool sym) {
  const int64_t tc = (n + GKM_T - 1) / GKM_T, trw = (rows + GKM_T - 1) / GKM_T;
  return sym ? tc * (tc + 1) / 2 : trw * tc;
}

hipError_t launch_gram_gkm(const uint32_t *words, int pmax, int l, bool rc, int64_t n, int64_t row0,
                           int64_t row1, bool sym, const GkmWeights &wt, const OutSpec &o,
                           hipStream_t s) {
  const int64_t rows = row1 - row0;
  if (rows <= 0 || n <= 0) return hipSuccess;
  if (pmax < 1 || pmax > 256 || l < 1 || l > 16) return hipErrorInvalidValue;
  if (sym && (row0 != 0 || rows != n)) return hipErrorInvalidValue;
  if (rc && l > 15) return hipErrorInvalidValue;  // rc(A^16) would be KMG_INVALID
  const int64_t tiles = gkm_tiles(n, rows, sym);
  if (tiles >= KMG_GKM_MAX_TILES) return hipErrorInvalidValue;  // AQL grid size is 32-bit
  const int pp = (pmax + 3) & ~3;
  const size_t lds =
      sizeof(uint32_t) * (size_t)((rc ? 3 : 2) * GKM_T * pp + GKM_WTAB + 2 + GKM_T * GKM_RES_LD);
  const dim3 grid((unsigned)tiles);
  const int64_t tiles_c = (n + GKM_T - 1) / GKM_T;
#define KMG_GKM_LAUNCH(NQ_)                                                                        \
  do {                                                                                             \
    auto kern = gram_gkm_kernel<NQ_, false, false>;                                                \
    if (sym) kern = rc ? gram_gkm_kernel<NQ_, true, true> : gram_gkm_kernel<NQ_, true, false>;     \
    else if (rc) kern = gram_gkm_kernel<NQ_, false, true>;                                         \
    hipLaunchKernelGGL(kern, grid, dim3(256), lds, s, words, pmax, l, n, row0, rows, tiles_c, wt,  \
                       o);                                                                         \
  } while (0)
  const int nq = (pmax + 31) / 32;  // row words a lane
  if (nq <= 1) KMG_GKM_LAUNCH(1);
  else if (nq == 2) KMG_GKM_LAUNCH(2);
  else if (nq == 3) KMG_GKM_LAUNCH(3);
  else if (nq == 4) KMG_GKM_LAUNCH(4);
  else if (nq <= 6) KMG_GKM_LAUNCH(6);
  else KMG_GKM_LAUNCH(8);
#undef KMG_GKM_LAUNCH
  return hipGetLastError();
}

hipError_t launch_gkm_diag(const uint32_t *words, int pmax, int l, bool rc, int64_t n,
                           const GkmWeights &wt, double *diagv, double *dsq, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  if (pmax < 1 || pmax > 256 || l < 1 || l > 16 || (rc && l > 15)) return hipErrorInvalidValue;
  const size_t lds = sizeof(uint32_t) * (size_t)(4 * pmax + GKM_WTAB);
  hipLaunchKernelGGL(rc ? gkm_diag_kernel<true> : gkm_diag_kernel<false>,
                     dim3((unsigned)((n + 3) / 4)), dim3(256), lds, s, words, pmax, l, n, wt, diagv,
                     dsq);
  return hipGetLastError();
}

}  // namespace kmg
