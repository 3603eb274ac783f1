// kmg_score.hip — score new sequences against a fitted model without a Gram block.
//
// Serves the prediction step of the reference's learners (KRR.py:43-56, SVM.py:99-111):
// f(q) = sum_t beta_t K(q, x_t) + b.  Spectrum (get_spectrum_K, kernels.py:28-47) and
// mismatch (get_mismatch_K, kernels.py:196-217) are inner products of explicit feature
// maps over the 4^k k-mers, so f(q) = sum_{windows a of q} U[q_a] + b for one table U of
// 4^k doubles built once from the training rows:
//   (1) vtab:       V[u] = sum_t beta_t #{valid windows of x_t equal to u}, from the exact-key
//                   posting index (copies = 1)
//   (2) butterfly:  mismatch only, U = sum_h w[h] E_h V, (E_h V)[z] = sum of V over the k-mers
//                   at Hamming distance exactly h of z, by the digit DP T_h += S_p T_{h-1}
//   (3) score:      one wave a query, P table reads
//
// Reproducibility.  The order of the entries inside a posting list is unspecified
// (kmg_index.hip), so (1) does not add doubles: every beta_t enters as a 128-bit fixed-point
// integer (90 fraction bits below the binade of max |beta|, made on the host) and the list
// sums are integer sums, exact in any order; V[u] is that integer rounded to double once.
// (2) and (3) add doubles in an order fixed by the launch geometry alone.  No atomics.
#include "kmg_internal.h"

namespace kmg {

// ------------------------------------------------------------------ (1) weight table
struct Fix128 {
  uint64_t lo;
  int64_t hi;
};
__device__ __forceinline__ void fix_add(Fix128 &a, uint64_t lo, int64_t hi) {
  const uint64_t s = a.lo + lo;
  a.hi += hi + (s < lo ? 1 : 0);
  a.lo = s;
}
// the integer hi * 2^64 + lo, rounded to nearest even once, times 2^e
__device__ __forceinline__ double fix_to_double(Fix128 a, int e) {
  const bool neg = a.hi < 0;
  uint64_t lo = a.lo, hi = (uint64_t)a.hi;
  if (neg) {
    lo = ~lo + 1;
    hi = ~hi + (lo == 0 ? 1 : 0);
  }
  double v;
  if (hi == 0) {
    v = (double)lo;  // one correctly rounded conversion
  } else {
    // 64 leading bits with the dropped ones folded into a sticky last bit: the uint64 ->
    // double conversion then rounds as the full 128-bit integer would
    const int sh = 64 - __clzll((long long)hi);
    const uint64_t top = (hi << (64 - sh)) | (lo >> sh);
    const uint64_t sticky = (lo << (64 - sh)) != 0 ? 1 : 0;
    v = ldexp((double)(top | sticky), sh);
  }
  return ldexp(neg ? -v : v, e);
}

// G lanes a key (1, 64 or 256): the key's lists of every chunk, entries strided over the lanes
template <int G>
__global__ __launch_bounds__(256) void score_vtab_kernel(IndexGeom g,
                                                         const uint32_t *__restrict__ off,
                                                         const uint16_t *__restrict__ ent,
                                                         const uint64_t *__restrict__ fix,
                                                         int scale_exp, double *__restrict__ V) {
  __shared__ Fix128 part[4];
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t key = t / G;
  const int sub = (int)(t % G);
  Fix128 acc{0, 0};
  if (key < (int64_t)g.nkeys) {
    for (int ch = 0; ch < g.nchunks; ++ch) {
      const int64_t bin = (int64_t)ch * g.nkeys + key;
      const uint32_t b = off[bin], e = off[bin + 1];
      const int64_t row0 = (int64_t)ch * g.chunk;
      for (uint32_t x = b + sub; x < e; x += G) {
        const int64_t row = row0 + ent[x];
        fix_add(acc, fix[2 * row], (int64_t)fix[2 * row + 1]);
      }
    }
  }
  if (G > 1) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1)
      fix_add(acc, __shfl_xor((unsigned long long)acc.lo, d, 64),
              (int64_t)__shfl_xor((unsigned long long)acc.hi, d, 64));
  }
  if (G == 256) {
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0)
      for (int w = 1; w < 4; ++w) fix_add(acc, part[w].lo, part[w].hi);
  }
  if (sub == 0 && key < (int64_t)g.nkeys) V[key] = fix_to_double(acc, scale_exp);
}

hipError_t launch_score_vtab(const IndexGeom &g, const uint32_t *off, const uint16_t *ent,
                             const uint64_t *fix, int scale_exp, double *V, hipStream_t s) {
  const int64_t nk = g.nkeys;
  // lists average n * pmax / 4^k entries: a workgroup a key up to k = 6, a wave up to k = 9,
  // a thread from k = 10 (under one entry a list at the sizes a single GPU holds)
  if (g.k <= 6)
    hipLaunchKernelGGL((score_vtab_kernel<256>), dim3((unsigned)nk), dim3(256), 0, s, g, off, ent,
                       fix, scale_exp, V);
  else if (g.k <= 9)
    hipLaunchKernelGGL((score_vtab_kernel<64>), dim3((unsigned)((nk + 3) / 4)), dim3(256), 0, s, g,
                       off, ent, fix, scale_exp, V);
  else
    hipLaunchKernelGGL((score_vtab_kernel<1>), dim3((unsigned)((nk + 255) / 256)), dim3(256), 0, s,
                       g, off, ent, fix, scale_exp, V);
  return hipGetLastError();
}

// ------------------------------------------------------------------ (2) Hamming butterfly
// One launch takes tg <= t digits [lo, lo + tg) (digit 0 = the last letter, the lowest two
// bits).  A tile is H values of the digits above, all 4^tg values of the launch's digits and
// a block of B consecutive values of the digits below, H * B = hb: every global row of the
// tile is B * 8 >= 64 contiguous bytes (the lowest group, lo = 0, is wholly contiguous).
// All nt = min(2m, k) + 1 DP tables of the tile sit in LDS; element e = (hh * 4^tg + mid) * B
// + low of table h at word h * tep + e + (e >> psh) * pad.  The digit passes own one
// butterfly (the four letters of one digit, every table) a thread, so a pass needs no
// barrier inside it.  Padding: lo = 0 (strides 1, 4, 16, 64) psh 2 pad 1 -- the four
// letters of a stride-1 butterfly in four banks, at most 2-way conflicts; lo > 0 (strides
// B, 4B, ...) psh 5 pad 8 -- conflict-free for B = 8 and 16 (64-bit LDS reads, 32 lanes a
// pass over 32 bank pairs).
struct ButterflyGeom {
  int k, nt, lo, tg, B, H, psh, pad, tep;
  int first, last;  // first: T_1.. are zero (not read); last: U = sum_h w[h] T_h, no T written
  double w[5];
};

__host__ __device__ __forceinline__ int bf_phys(int e, int psh, int pad) { return e + (e >> psh) * pad; }

template <int NT>
__global__ __launch_bounds__(256) void score_butterfly_kernel(ButterflyGeom bg,
                                                              double *__restrict__ T,
                                                              double *__restrict__ U) {
  extern __shared__ __align__(16) double tile[];
  const int M = 1 << (2 * bg.tg);
  const int te = M * bg.B * bg.H;
  const int64_t tsz = (int64_t)1 << (2 * bg.k);
  const int64_t nlb = ((int64_t)1 << (2 * bg.lo)) / bg.B;
  const int64_t lb = blockIdx.x % nlb, high0 = (blockIdx.x / nlb) * bg.H;
  const int bshift = __ffs(bg.B) - 1;
  auto global_index = [&](int e) -> int64_t {
    const int low = e & (bg.B - 1), mid = (e >> bshift) & (M - 1), hh = e >> (bshift + 2 * bg.tg);
    return ((high0 + hh) << (2 * (bg.lo + bg.tg))) | ((int64_t)mid << (2 * bg.lo)) |
           (lb * bg.B + low);
  };
  for (int e = threadIdx.x; e < te; e += 256) {
    const int64_t z = global_index(e);
    const int pe = bf_phys(e, bg.psh, bg.pad);
#pragma unroll
    for (int h = 0; h < NT; ++h)
      tile[h * bg.tep + pe] = (bg.first && h > 0) ? 0.0 : T[h * tsz + z];
  }
  __syncthreads();
  for (int j = 0; j < bg.tg; ++j) {
    const int sshift = bshift + 2 * j;  // butterfly stride B * 4^j
    for (int r = threadIdx.x; r < te / 4; r += 256) {
      const int e0 = ((r >> sshift) << (sshift + 2)) | (r & ((1 << sshift) - 1));
      int pe[4];
      double a[NT][4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        pe[c] = bf_phys(e0 + (c << sshift), bg.psh, bg.pad);
#pragma unroll
        for (int h = 0; h < NT; ++h) a[h][c] = tile[h * bg.tep + pe[c]];
      }
      // T_h += S T_{h-1}: the three other letters, summed directly in letter order
#pragma unroll
      for (int h = NT - 1; h >= 1; --h) {
        tile[h * bg.tep + pe[0]] = a[h][0] + ((a[h - 1][1] + a[h - 1][2]) + a[h - 1][3]);
        tile[h * bg.tep + pe[1]] = a[h][1] + ((a[h - 1][0] + a[h - 1][2]) + a[h - 1][3]);
        tile[h * bg.tep + pe[2]] = a[h][2] + ((a[h - 1][0] + a[h - 1][1]) + a[h - 1][3]);
        tile[h * bg.tep + pe[3]] = a[h][3] + ((a[h - 1][0] + a[h - 1][1]) + a[h - 1][2]);
      }
    }
    __syncthreads();
  }
  for (int e = threadIdx.x; e < te; e += 256) {
    const int64_t z = global_index(e);
    const int pe = bf_phys(e, bg.psh, bg.pad);
    if (bg.last) {
      double u = bg.w[0] * tile[pe];
#pragma unroll
      for (int h = 1; h < NT; ++h) u += bg.w[h] * tile[h * bg.tep + pe];
      U[z] = u;
    } else {
#pragma unroll
      for (int h = 0; h < NT; ++h) T[h * tsz + z] = tile[h * bg.tep + pe];
    }
  }
}

// digits a launch: 4 where the padded tile of nt tables fits lds_max, else fewer; hb = rows
// of the tile beside its 4^t digit values (16 entries = 128-byte segments; 8 = 64 bytes at
// nt = 5, where 16 would need 200 KB)
// (each table of the tile takes 5/4 of its elements plus at most 8 words of padding, tep in
// launch_score_butterfly).  gfx950's 160 KB always gives t = 4.  t never goes below 2 (at
// most 14 KB): a group above the lowest then has >= 16 values below it, so every global row
// of a tile keeps its >= 64 bytes; a device with less LDS fails the launch loudly.
int score_tile_digits(int nt, size_t lds_max, int *hb) {
  *hb = nt <= 3 ? 16 : 8;
  int t = 4;
  while (t > 2 &&(size_t)nt * ((size_t)(*hb << (2 * t)) * 5 / 4 + 8) * sizeof(double) > lds_max)
    --t;
  return t;
}

hipError_t launch_score_butterfly(double *T, int k, int nt, int lo, int tg, int hb, bool first,
                                  bool last, const double *w, double *U, hipStream_t s) {
  ButterflyGeom bg{};
  bg.k = k;
  bg.nt = nt;
  bg.lo = lo;
  bg.tg = tg;
  const int64_t below = (int64_t)1 << (2 * lo), above = (int64_t)1 << (2 * (k - lo - tg));
  bg.B = (int)(below < hb ? below : hb);
  bg.H = (int)(above < hb / bg.B ? above : hb / bg.B);
  bg.psh = lo == 0 ? 2 : 5;
  bg.pad = lo == 0 ? 1 : 8;
  const int te = (bg.B * bg.H) << (2 * tg);
  bg.tep = bf_phys(te, bg.psh, bg.pad) + bg.pad;
  bg.first = first;
  bg.last = last;
  for (int h = 0; h < 5; ++h) bg.w[h] = h < nt ? w[h] : 0.0;
  const int64_t tiles = (below / bg.B) * (above / bg.H);
  const size_t lds = (size_t)nt * bg.tep * sizeof(double);
  const dim3 grid((unsigned)tiles);
  switch (nt) {
    case 1: hipLaunchKernelGGL((score_butterfly_kernel<1>), grid, dim3(256), lds, s, bg, T, U); break;
    case 2: hipLaunchKernelGGL((score_butterfly_kernel<2>), grid, dim3(256), lds, s, bg, T, U); break;
    case 3: hipLaunchKernelGGL((score_butterfly_kernel<3>), grid, dim3(256), lds, s, bg, T, U); break;
    case 4: hipLaunchKernelGGL((score_butterfly_kernel<4>), grid, dim3(256), lds, s, bg, T, U); break;
    case 5: hipLaunchKernelGGL((score_butterfly_kernel<5>), grid, dim3(256), lds, s, bg, T, U); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

// ------------------------------------------------------------------ (3) scorer
// One wave a query, four a workgroup: the 2-bit record staged in LDS, lanes take the windows
// a = lane, lane + 64, ... in order, then a fixed xor tree over the wave (every lane ends
// with the same bits), the K_qq scaling and the bias; the four results leave in one store.
__global__ __launch_bounds__(256) void score_kernel(Packed pk, int64_t nq, int k, int P,
                                                    const double *__restrict__ U,
                                                    const double *__restrict__ dsq, double bias,
                                                    double *__restrict__ out) {
  extern __shared__ __align__(16) uint32_t srec_all[];  // [4][ldp]
  __shared__ double res[4];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t q = (int64_t)blockIdx.x * 4 + wave;
  uint32_t *srec = srec_all + wave * pk.ldp;
  if (q < nq) {
    const uint32_t *rec = pk.w + q * pk.ldp;
    for (int t = lane; t < (int)pk.ldp; t += 64) srec[t] = rec[t];
  }
  __syncthreads();
  double s = 0.0;
  if (q < nq)
    for (int a = lane; a < P; a += 64) {
      const uint32_t code = pk_window(srec, pk.cw, a, k);
      if (code != KMG_INVALID) s += U[code];
    }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
  if (lane == 0 && q < nq) res[wave] = dsq ? s / dsq[q] + bias : s + bias;
  __syncthreads();
  const int64_t qo = (int64_t)blockIdx.x * 4 + threadIdx.x;
  if (threadIdx.x < 4 && qo < nq) out[qo] = res[threadIdx.x];
}

hipError_t launch_score(const Packed &pk, int64_t nq, int k, int P, const double *U,
                        const double *dsq, double bias, double *out, hipStream_t s) {
  if (nq == 0) return hipSuccess;
  const size_t lds = (size_t)4 * pk.ldp * sizeof(uint32_t);
  hipLaunchKernelGGL(score_kernel, dim3((unsigned)((nq + 3) / 4)), dim3(256), lds, s, pk, nq, k, P,
                     U, dsq, bias, out);
  return hipGetLastError();
}

}  // namespace kmg
