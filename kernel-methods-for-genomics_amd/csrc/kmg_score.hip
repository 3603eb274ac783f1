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
//
// Section (4) at the end is the gapped k-mer model's table scorer (kmg_gkm_scorer_*): its own
// weight-table kernel, split by words, with 128-bit integer atomics, and its own scoring
// kernels, several queries a wave; the butterfly (2) is shared.  Section (5) is that model's
// substitution map (kmg_gkm_scorer_mutate*): the score difference of every single-letter
// substitution of a query, one lane a (position, letter), from the same table.
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

// ------------------------------------------------------------------ (4) gkm table scorer
// The gapped k-mer model (kmg_gkm_scorer_*) as the same kind of table:
//   V[v] = sum_t beta_t sum_b w_t[b] [x_t word b = v]     (vtab; both strands: V[v] + V[rc(v)])
//   U    = sum_{m <= d} c[m] E_m V                        (the butterfly above, nt = d + 1)
//   f(q) = sum_a u_q[a] U[q_a] (/ sqrt(K_qq)) + bias      (score)
// The work of (vtab) is split by words: a workgroup stages a batch of records, one lane takes
// one word and adds beta_t w_t[b], a 128-bit integer, into the word's table entry with two
// 64-bit integer atomics.  Integer sums are exact in any order, so the table does not depend
// on the grid, the batch or the order the atomics land in.  Fixed point: KMG_GKS_FRAC = 80
// fraction bits below 2^E > max |beta|, so |beta_t| 2^(80 - E) < 2^80 and
//   2 strands * 255 * (fewer than 2^36 words, KMG_GKS_MAX_WORDS) * 2^80 < 2^125 < 2^127;
// a beta is cut to that grid once on the host (less than 2^(E - 80) off).
// Rows of any length: a record is staged in segments of GKS_SEG word starts, in the record's
// own layout (code words, then mask words), so pk_window reads a segment as it reads a record.
constexpr int GKS_SEG = 2048;
constexpr int GKS_CW = GKS_SEG / 16 + 2;
constexpr int GKS_MW = GKS_SEG / 32 + 2;

// word i of the staged form of segment seg: code words [0, cws), mask words [cws, cws + mws);
// past the record: no letters, every one of them masked
__device__ __forceinline__ uint32_t gks_word(const uint32_t *rec, int cw, int mw, int cws, int seg,
                                             int i) {
  if (i < cws) {
    const int s = seg * (GKS_SEG / 16) + i;
    return s < cw ? rec[s] : 0u;
  }
  const int s = seg * (GKS_SEG / 32) + (i - cws);
  return s < mw ? rec[cw + s] : 0xFFFFFFFFu;
}

// *p (low limb, high limb) += (lo, hi) mod 2^128: the carry out of the low limb is read off
// the value the first atomic returns, so every interleaving of such adds gives the exact sum
template <typename T>
__device__ __forceinline__ void gks_atomic_add(T *p, uint64_t lo, uint64_t hi) {
  const uint64_t old = atomicAdd(p, (unsigned long long)lo);
  hi += (old + lo < lo) ? 1 : 0;
  if (hi != 0) atomicAdd(p + 1, (unsigned long long)hi);
}

// PRIV (l <= 6): the whole table, 16 bytes a key, private to the workgroup in LDS (ds 64-bit
// atomics), flushed once with global atomics; else global atomics a word.  A batch is B
// (row, segment) items of ps = min(P, GKS_SEG) word starts each.
template <bool PRIV>
__global__ __launch_bounds__(256) void gkm_vtab_kernel(Packed pk, int mw, int64_t n, int l, int P,
                                                       int B, const uint8_t *__restrict__ wts,
                                                       int64_t ldw,
                                                       const uint64_t *__restrict__ fix,
                                                       unsigned long long *__restrict__ tab) {
  extern __shared__ __align__(16) unsigned long long gks_priv[];  // [2 * 4^l] (PRIV), then records
  const int nkeys = 1 << (2 * l);
  uint32_t *srec = (uint32_t *)(gks_priv + (PRIV ? 2 * nkeys : 0));
  const int cws = min(pk.cw, GKS_CW), mws = min(mw, GKS_MW), rs = cws + mws;
  const int nseg = (P + GKS_SEG - 1) / GKS_SEG, ps = min(P, GKS_SEG);
  const int64_t nitems = n * nseg;
  if (PRIV) {
    for (int t = threadIdx.x; t < 2 * nkeys; t += 256) gks_priv[t] = 0;
  }
  for (int64_t it0 = (int64_t)blockIdx.x * B; it0 < nitems; it0 += (int64_t)gridDim.x * B) {
    const int nb = (int)min((int64_t)B, nitems - it0);
    __syncthreads();  // the table is cleared / the last batch is done with srec
    for (int t = threadIdx.x; t < nb * rs; t += 256) {
      const int b = t / rs;
      const int64_t row = (it0 + b) / nseg;
      srec[t] = gks_word(pk.w + row * pk.ldp, pk.cw, mw, cws, (int)((it0 + b) % nseg), t - b * rs);
    }
    __syncthreads();
    for (int t = threadIdx.x; t < nb * ps; t += 256) {
      const int b = t / ps, a = t - b * ps;
      const int64_t row = (it0 + b) / nseg;
      const int ga = (int)((it0 + b) % nseg) * GKS_SEG + a;  // the word's start in its row
      if (ga >= P) continue;
      const uint32_t code = pk_window(srec + b * rs, cws, a, l);
      if (code == KMG_INVALID) continue;
      const uint64_t wv = wts ? wts[row * ldw + ga] : 1;
      // beta_t * w (two's complement, mod 2^128)
      const uint64_t lo = fix[2 * row], hi = fix[2 * row + 1];
      const uint64_t plo = lo * wv, phi = hi * wv + __umul64hi(lo, wv);
      if ((plo | phi) == 0) continue;
      if (PRIV)
        gks_atomic_add(gks_priv + 2 * (size_t)code, plo, phi);
      else
        gks_atomic_add(tab + 2 * (size_t)code, plo, phi);
    }
  }
  if (PRIV) {
    __syncthreads();
    for (int key = threadIdx.x; key < nkeys; key += 256) {
      const uint64_t lo = gks_priv[2 * key], hi = gks_priv[2 * key + 1];
      if ((lo | hi) != 0) gks_atomic_add(tab + 2 * (size_t)key, lo, hi);
    }
  }
}

// reverse complement of a word of l letters (A<->T, C<->G: 3 - letter; letters reversed)
__device__ __forceinline__ uint32_t gks_rc(uint32_t v, int l) {
  uint32_t x = ~v;
  x = ((x >> 2) & 0x33333333u) | ((x & 0x33333333u) << 2);
  x = ((x >> 4) & 0x0F0F0F0Fu) | ((x & 0x0F0F0F0Fu) << 4);
  x = __builtin_bswap32(x);
  return x >> (32 - 2 * l);
}

// T_0[v] = the table entry rounded to double once; rc: the integer sum of the entries of v
// and rc(v) rounded once (a palindrome counts on both strands, so its own entry twice)
__global__ __launch_bounds__(256) void gkm_vconv_kernel(const unsigned long long *__restrict__ tab,
                                                        int l, int rc, int scale_exp,
                                                        double *__restrict__ T0) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= ((int64_t)1 << (2 * l))) return;
  Fix128 a{tab[2 * v], (int64_t)tab[2 * v + 1]};
  if (rc) {
    const uint32_t r = gks_rc((uint32_t)v, l);
    fix_add(a, tab[2 * (size_t)r], (int64_t)tab[2 * (size_t)r + 1]);
  }
  T0[v] = fix_to_double(a, scale_exp);
}

__global__ __launch_bounds__(256) void gkm_tab_clear_kernel(unsigned long long *__restrict__ tab,
                                                            int64_t nwords) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t < nwords) tab[t] = 0;
}

// both strands: the butterfly adds the letters of a digit in letter order, which the reverse
// complement permutes, so U[z] and U[rc(z)] can differ in the last bits; the entry of the
// smaller of z, rc(z) is taken for both (entries with z <= rc(z) are only read)
__global__ __launch_bounds__(256) void gkm_usym_kernel(double *__restrict__ U, int l) {
  const int64_t z = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (z >= ((int64_t)1 << (2 * l))) return;
  const uint32_t r = gks_rc((uint32_t)z, l);
  if ((int64_t)r < z) U[z] = U[r];
}

int gkm_vtab_batch(int P) {
  // 1024 word starts a batch (four a lane) where the rows are short, 32 rows at the most
  const int ps = P < GKS_SEG ? P : GKS_SEG;
  int B = (1024 + ps - 1) / ps;
  return B < 1 ? 1 : B > 32 ? 32 : B;
}

hipError_t launch_gkm_vtab(const Packed &pk, int mw, int64_t n, int l, int P, const uint8_t *wts,
                           int64_t ldw, const uint64_t *fix, uint64_t *tab, hipStream_t s) {
  const int64_t nkeys = (int64_t)1 << (2 * l);
  hipLaunchKernelGGL(gkm_tab_clear_kernel, dim3((unsigned)((2 * nkeys + 255) / 256)), dim3(256), 0, s,
                     (unsigned long long *)tab, 2 * nkeys);
  if (n == 0 || P <= 0) return hipGetLastError();  // no word anywhere: the table stays zero
  const int B = gkm_vtab_batch(P);
  const int cws = pk.cw < GKS_CW ? pk.cw : GKS_CW, mws = mw < GKS_MW ? mw : GKS_MW;
  const int nseg = (P + GKS_SEG - 1) / GKS_SEG;
  const int64_t nbatch = (n * nseg + B - 1) / B;
  const size_t rec_lds = (size_t)B * (cws + mws) * sizeof(uint32_t);
  if (l <= 6) {
    // a workgroup flushes 4^l entries: give it at least four words a key before it does
    const int64_t words = n * (int64_t)P;
    int64_t grid = words / (4 * nkeys);
    grid = grid < 1 ? 1 : grid > 256 ? 256 : grid;
    if (grid > nbatch) grid = nbatch;
    hipLaunchKernelGGL((gkm_vtab_kernel<true>), dim3((unsigned)grid), dim3(256),
                       (size_t)nkeys * 16 + rec_lds, s, pk, mw, n, l, P, B, wts, ldw, fix,
                       (unsigned long long *)tab);
  } else {
    const int64_t grid = nbatch < 65536 ? nbatch : 65536;
    hipLaunchKernelGGL((gkm_vtab_kernel<false>), dim3((unsigned)grid), dim3(256), rec_lds, s, pk, mw,
                       n, l, P, B, wts, ldw, fix, (unsigned long long *)tab);
  }
  return hipGetLastError();
}

hipError_t launch_gkm_vconv(const uint64_t *tab, int l, bool rc, int scale_exp, double *T0,
                            hipStream_t s) {
  const int64_t nkeys = (int64_t)1 << (2 * l);
  hipLaunchKernelGGL(gkm_vconv_kernel, dim3((unsigned)((nkeys + 255) / 256)), dim3(256), 0, s,
                     (const unsigned long long *)tab, l, rc ? 1 : 0, scale_exp, T0);
  return hipGetLastError();
}

hipError_t launch_gkm_usym(double *U, int l, hipStream_t s) {
  const int64_t nkeys = (int64_t)1 << (2 * l);
  hipLaunchKernelGGL(gkm_usym_kernel, dim3((unsigned)((nkeys + 255) / 256)), dim3(256), 0, s, U, l);
  return hipGetLastError();
}

// G lanes a query, 256 / G queries a workgroup (G = 8, 16, 64): the records, and the weights
// where given, staged in LDS; lane j of a query takes its words a = j, j + G, ... in
// ascending order, each product u[a] * U[code] rounded before it is added; a fixed xor tree of
// width G (every lane of the group ends with the same bits); / sqrt(K_qq), + bias; the
// workgroup's results leave in one store.  P <= 1024 words (the host picks G from P).
template <int G>
__global__ __launch_bounds__(256) void gkm_score_kernel(Packed pk, int64_t nq, int l, int P,
                                                        const uint8_t *__restrict__ wts,
                                                        int64_t ldw, const double *__restrict__ U,
                                                        const double *__restrict__ dsq, double bias,
                                                        double *__restrict__ out) {
  constexpr int QW = 256 / G;
  extern __shared__ __align__(16) uint32_t gks_q[];  // [QW][ldp] records, then [QW][pw] weight bytes
  __shared__ double res[QW];
  const int pw = (P + 3) & ~3;
  uint8_t *swt = (uint8_t *)(gks_q + QW * pk.ldp);
  const int64_t q0 = (int64_t)blockIdx.x * QW;
  const int nqw = (int)min((int64_t)QW, nq - q0);
  for (int t = threadIdx.x; t < nqw * (int)pk.ldp; t += 256) gks_q[t] = pk.w[q0 * pk.ldp + t];
  if (wts)
    for (int t = threadIdx.x; t < nqw * P; t += 256) {
      const int qi = t / P, a = t - qi * P;
      swt[qi * pw + a] = wts[(q0 + qi) * ldw + a];
    }
  __syncthreads();
  const int qi = threadIdx.x / G, sub = threadIdx.x % G;
  double s = 0.0;
  if (qi < nqw) {
    const uint32_t *srec = gks_q + qi * pk.ldp;
    for (int a = sub; a < P; a += G) {
      const uint32_t code = pk_window(srec, pk.cw, a, l);
      if (code == KMG_INVALID) continue;
      if (wts)
        s += (double)swt[qi * pw + a] * U[code];
      else
        s += U[code];
    }
  }
#pragma unroll
  for (int d = G / 2; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
  if (sub == 0 && qi < nqw) res[qi] = dsq ? s / dsq[q0 + qi] + bias : s + bias;
  __syncthreads();
  if (threadIdx.x < nqw) out[q0 + threadIdx.x] = res[threadIdx.x];
}

// the workgroup-wide form, rows of any length: one query a workgroup, the record staged a
// segment at a time; lane t takes the words a = t, t + 256, ... of every segment in ascending
// order, then the xor tree of each wave and the four wave sums added in wave order
__global__ __launch_bounds__(256) void gkm_score_wide_kernel(Packed pk, int mw, int64_t nq, int l,
                                                             int P, const uint8_t *__restrict__ wts,
                                                             int64_t ldw,
                                                             const double *__restrict__ U,
                                                             const double *__restrict__ dsq,
                                                             double bias, double *__restrict__ out) {
  __shared__ uint32_t srec[GKS_CW + GKS_MW];
  __shared__ uint8_t swt[GKS_SEG];
  __shared__ double part[4];
  const int64_t q = blockIdx.x;
  const uint32_t *rec = pk.w + q * pk.ldp;
  const int nseg = (P + GKS_SEG - 1) / GKS_SEG;
  double s = 0.0;
  for (int seg = 0; seg < nseg; ++seg) {
    const int a0 = seg * GKS_SEG, na = min(GKS_SEG, P - a0);
    __syncthreads();
    for (int t = threadIdx.x; t < GKS_CW + GKS_MW; t += 256)
      srec[t] = gks_word(rec, pk.cw, mw, GKS_CW, seg, t);
    if (wts)
      for (int t = threadIdx.x; t < na; t += 256) swt[t] = wts[q * ldw + a0 + t];
    __syncthreads();
    for (int a = threadIdx.x; a < na; a += 256) {
      const uint32_t code = pk_window(srec, GKS_CW, a, l);
      if (code == KMG_INVALID) continue;
      if (wts)
        s += (double)swt[a] * U[code];
      else
        s += U[code];
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double t = ((part[0] + part[1]) + part[2]) + part[3];
    out[q] = dsq ? t / dsq[q] + bias : t + bias;
  }
}

// lanes a query from the word bound P alone (ldc in both the host and the device form):
// at most 4 words a lane on 8 lanes, 8 on 16, 16 on a wave, then a workgroup
int gkm_score_lanes(int P) { return P <= 32 ? 8 : P <= 128 ? 16 : P <= 1024 ? 64 : 256; }

hipError_t launch_gkm_score(const Packed &pk, int mw, int64_t nq, int l, int P, int G,
                            const uint8_t *wts, int64_t ldw, const double *U, const double *dsq,
                            double bias, double *out, hipStream_t s) {
  if (nq == 0) return hipSuccess;
  if (G != 256 && P > 1024) return hipErrorInvalidValue;  // (the staged record is the whole row)
  const int qw = G == 256 ? 1 : 256 / G;
  const dim3 grid((unsigned)((nq + qw - 1) / qw));
  const size_t lds = (size_t)qw * (pk.ldp * sizeof(uint32_t) + (wts ? (size_t)((P + 3) & ~3) : 0));
  switch (G) {
    case 8: hipLaunchKernelGGL((gkm_score_kernel<8>), grid, dim3(256), lds, s, pk, nq, l, P, wts, ldw, U, dsq, bias, out); break;
    case 16: hipLaunchKernelGGL((gkm_score_kernel<16>), grid, dim3(256), lds, s, pk, nq, l, P, wts, ldw, U, dsq, bias, out); break;
    case 64: hipLaunchKernelGGL((gkm_score_kernel<64>), grid, dim3(256), lds, s, pk, nq, l, P, wts, ldw, U, dsq, bias, out); break;
    case 256: hipLaunchKernelGGL(gkm_score_wide_kernel, grid, dim3(256), 0, s, pk, mw, nq, l, P, wts, ldw, U, dsq, bias, out); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

// ------------------------------------------------------------------ (5) gkm substitution map
// kmg_gkm_scorer_mutate*: out[q][i][b] = S_b(i) - R(i), the raw score of q with letter b at
// position i minus the raw score of q (deltaSVM's sum of l-mer weight differences):
//   S_b(i) = sum over the words a that cover i, max(0, i - l + 1) <= a <= min(i, P - 1), whose
//            other letters are all A/C/G/T, in ascending a from +0.0, of u[a] * U[word a with
//            its letter at offset i - a replaced by b] (the product rounded before the add)
//   R(i)   = S_{q_i}(i) where q_i is A/C/G/T, +0.0 where it is not
// The order of the adds is the definition's, so no bit depends on the launch geometry.
// One lane a (position, letter), four lanes a position; an item is S consecutive positions of
// one query (S = 8, 16, 32, 64 from ldc alone), 64 / S items a workgroup of 256 lanes; a row
// of any length is a run of items.  Phase 1: an item's lanes write its S + l - 1 words to LDS,
// 8 bytes a word: the 2l-bit code; the mask of its non-ACGT letters (bit o = the letter at
// offset o) in bits 0..11, bit 15 for a word that starts before the row or ends after it, the
// weight byte in bits 16..23; and the S letters of its positions (4 = not A/C/G/T or past the
// end).  Phase 2: lane (i, b) reads the l words a = i - l + 1 + j, j = 0..l - 1 (the four
// lanes of a position the same 8 bytes, neighbouring positions neighbouring words), clears the
// two code bits 2j, 2j + 1 of position i and sets b, issues its up to 12 table loads, then
// adds them in ascending j.  R(i) is the sum of the lane of the quad whose b is q_i, fetched
// by a lane permute.  No cross-lane sum; an item's results leave in one store of 32 S bytes.
constexpr int GKM_MUT_LMAX = 12;

int gkm_mutate_block(int64_t ldc) { return ldc <= 8 ? 8 : ldc <= 16 ? 16 : ldc <= 32 ? 32 : 64; }

// L = l (the phase-2 loop is unrolled over it, its table values in registers); W: weighted;
// items < 2^31 (the host checks)
template <int L, bool W>
__global__ __launch_bounds__(256) void gkm_mutate_kernel(Packed pk, const int32_t *__restrict__ lens,
                                                         uint32_t items, int ldc, int ssh, int npos,
                                                         const uint8_t *__restrict__ wts,
                                                         int64_t ldw, const double *__restrict__ U,
                                                         double *__restrict__ out) {
  extern __shared__ __align__(8) uint2 mut_words[];  // [64 / S][S + l - 1], then [64 / S][S] letters
  constexpr int l = L;
  const int S = 1 << ssh, nw = S + l - 1, lanes = 4 * S;
  uint8_t *slet = (uint8_t *)(mut_words + (64 >> ssh) * nw);
  const int iw = threadIdx.x >> (ssh + 2), t = threadIdx.x & (lanes - 1);
  const uint32_t items_row = (uint32_t)(npos + S - 1) >> ssh;
  const uint32_t it = blockIdx.x * (64u >> ssh) + iw;
  const bool live = it < items;
  const int64_t q = live ? it / items_row : 0;
  const int p0 = live ? (int)(it % items_row) << ssh : 0;
  const int len = live ? min(max(lens[q], 0), ldc) : 0;
  if (live) {
    const uint32_t *rec = pk.w + q * pk.ldp;
    for (int w = t; w < nw; w += lanes) {
      const int a = p0 - l + 1 + w;
      uint2 e = make_uint2(0u, 0x8000u);
      if (a >= 0 && a + l <= len) {  // (so no read leaves the record)
        const uint64_t v = ((uint64_t)rec[a >> 4] << 32) | rec[(a >> 4) + 1];
        e.x = (uint32_t)((v << (2 * (a & 15))) >> (64 - 2 * l));
        const int j = pk.cw + (a >> 5);
        const uint64_t m = ((((uint64_t)rec[j + 1]) << 32) | rec[j]) >> (a & 31);
        e.y = (uint32_t)(m & ((1u << l) - 1u));
        if (W) e.y |= (uint32_t)wts[q * ldw + a] << 16;
      }
      mut_words[iw * nw + w] = e;
    }
    if (t < S) {
      const int i = p0 + t;
      uint32_t c = 4;
      if (i < len && ((rec[pk.cw + (i >> 5)] >> (i & 31)) & 1u) == 0)
        c = (rec[i >> 4] >> (30 - 2 * (i & 15))) & 3u;
      slet[iw * S + t] = (uint8_t)c;
    }
  }
  __syncthreads();
  const int pi = t >> 2;
  const uint32_t b = t & 3;
  const uint2 *wd = mut_words + iw * nw + pi;
  // every lane loads (a word that does not count reads a table entry all the same: the index
  // is cut to the table, whatever its code bits hold); the adds alone are predicated
  constexpr uint32_t zmask = (1u << (2 * l)) - 1u;
  double v[L];
  uint32_t ok = 0;
#pragma unroll
  for (int j = 0; j < L; ++j) {
    const uint2 e = wd[j];  // word a = p0 + pi - (l - 1) + j: position i at its offset l - 1 - j
    bool good = live && ((e.y & 0xFFFFu) & ~(1u << (l - 1 - j))) == 0;
    if (W) good = good && (e.y >> 16) != 0;
    const uint32_t z = ((e.x & ~(3u << (2 * j))) | (b << (2 * j))) & zmask;
    v[j] = W ? (double)((e.y >> 16) & 0xFFu) * U[z] : U[z];
    ok |= good ? 1u << j : 0u;
  }
  double s = 0.0;
#pragma unroll
  for (int j = 0; j < L; ++j) s = ((ok >> j) & 1u) ? s + v[j] : s;
  const uint32_t qi = live ? slet[iw * S + pi] : 4u;
  const double r = __shfl(s, (int)(qi & 3u), 4);
  const int i = p0 + pi;
  if (live && i < npos) out[(q * npos + i) * 4 + b] = i < len ? s - (qi < 4 ? r : 0.0) : 0.0;
}

hipError_t launch_gkm_mutate(const Packed &pk, const int32_t *lens, int64_t nq, int64_t ldc, int l,
                             int64_t ld_out, const uint8_t *wts, int64_t ldw, const double *U,
                             double *out, hipStream_t s) {
  if (nq == 0 || ld_out == 0) return hipSuccess;
  if (l < 1 || l > GKM_MUT_LMAX || ld_out > 0x7FFFFFFF - 64) return hipErrorInvalidValue;
  const int S = gkm_mutate_block(ldc), ssh = __builtin_ctz(S), iw = 64 / S;
  const int64_t items = nq * ((ld_out + S - 1) / S);
  if (items > 0x7FFFFFFF) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((items + iw - 1) / iw));
  const size_t lds = (size_t)iw * ((size_t)(S + l - 1) * sizeof(uint2) + S);
#define KMG_MUT_CASE(LL)                                                                           \
  case LL:                                                                                         \
    if (wts)                                                                                       \
      hipLaunchKernelGGL((gkm_mutate_kernel<LL, true>), grid, dim3(256), lds, s, pk, lens,         \
                         (uint32_t)items, (int)ldc, ssh, (int)ld_out, wts, ldw, U, out);           \
    else                                                                                           \
      hipLaunchKernelGGL((gkm_mutate_kernel<LL, false>), grid, dim3(256), lds, s, pk, lens,        \
                         (uint32_t)items, (int)ldc, ssh, (int)ld_out, wts, ldw, U, out);           \
    break;
  switch (l) {
    KMG_MUT_CASE(1) KMG_MUT_CASE(2) KMG_MUT_CASE(3) KMG_MUT_CASE(4) KMG_MUT_CASE(5) KMG_MUT_CASE(6)
    KMG_MUT_CASE(7) KMG_MUT_CASE(8) KMG_MUT_CASE(9) KMG_MUT_CASE(10) KMG_MUT_CASE(11) KMG_MUT_CASE(12)
  }
#undef KMG_MUT_CASE
  return hipGetLastError();
}

}  // namespace kmg
