// kmg_gkmx.hip — the rectangular gapped k-mer kernel for rows of any length, on int8 MFMA
// (gfx950).
//
//   Kx[i][j] = sum_{a, b} h[ham(A_i[a:a+l], B_j[b:b+l])],  h[m] = C(l - m, k) for m <= d, else 0
//
// for two sequence sets A (na rows) and B (nb rows): the block K(queries x support vectors) of
// gkm-SVM prediction, and with A = B the square Gram of rows past kmg_gkm.hip's 256 words.  The
// word rules are KMG_GKM's (all windows of the whole row; a window holding a non-ACGT symbol
// counts nothing), except that T^16 is a word like any other: validity is a bit beside the
// word, not a marker value inside it.
//
// Word matches as a matrix product.  For 32 words of A_i and 32 words of B_j, one-hot operands
// X[a][(p, c)] = [letter p of word a is c] give (X_A X_B^T)[a][b] = l - ham(a, b): 4 l <= 64
// k-values, two v_mfma_i32_32x32x32_i8 steps (one at l <= 8).  Both operands hold 2 where the
// letter is, so an accumulator entry is 4 * matches: the byte offset into the LDS table
// hm[m] = h[l - m].  A word pair then costs one ds_read_b32 and one add.  hm[0] = h[l] = 0
// (d <= l - k < l), so an all-zero operand -- an invalid word, a word past the row's end, a
// letter position >= l -- counts nothing and needs no special case.
//
// gkmx_extract_kernel   packed records -> words [n][32 nblk] (0 where invalid) and validity
//                       bits [n][nblk], nblk = ceil(pmax / 32) blocks of 32 words a row.
// gram_gkmx_kernel<DIAG, TWO, RC, WT, PF>   one 256-thread workgroup a tile of 16 rows x 8 columns.
//   LDS     one chunk of 8 blocks (256 words) of every tile row and column, 4 B a word:
//           16 KB + 8 KB, their validity words (768 B), hm (80 B) and the int64 result tile
//           (1 KB): 26 KB whatever pmax is.  The chunk loops (A chunks outside, B chunks
//           inside; the A chunk is staged once a sweep of the B chunks) are workgroup-uniform.
//   waves   wave w owns the pairs (rows 4w .. 4w + 3) x (8 columns), whole.
//   lanes   lane = (word slot 0..31, half).  A lane expands its word's 4 letters of each MFMA
//           step into 4 dwords (16 k-values): step 0 takes letters 0..7 (half 0 letters 0..3,
//           half 1 letters 4..7), step 1 letters 8..15 (TWO, l > 8).  The word is left-aligned
//           first, so letter p sits at bits 31 - 2p, 30 - 2p for every l; the dword of a letter
//           position >= l is built from the lane constant 0 instead of 2.  The same expansion
//           serves both operands, so the lane / element -> k map is the same by construction.
//   sweep   for each A block the four rows' operands are expanded once (32 VGPRs) and stay in
//           registers while the wave walks the 8 columns' B blocks of the staged chunk: one
//           ds_read_b32 and one expansion a B block, then per row 1 or 2 MFMAs and the 16
//           lookups.  A B block whose 32 validity bits are all set skips the masking; one with
//           none set, or an A block with none set in all four rows, is skipped (wave-uniform:
//           the validity word is one LDS address a wave).
//   sums    the 16 lookups of an MFMA result are added in int32 (<= 16 * 12870) and that sum
//           goes into the pair's per-lane int64: an int32 never holds more than 16 adds.  One
//           xor-shuffle reduction a pair at the end; the raw value is exact in int64 and is
//           converted once to the output type.
//   DIAG    pairs (i, i): a tile is 8 rows, staged on both sides; wave w owns rows 2w, 2w + 1
//           and sweeps each against itself.  Writes sqrt(K_ii) (IEEE) for the normalisation.
//   RC      both strands (kmg_params.strands = 2):
//             K2(x, y) = K(x, y) + K(x, rc(y)) = sum_{a, b} (h[ham(x_a, y_b)] + h[ham(x_a, rc(y_b))])
//           rc = reverse complement (letters reversed, code c -> c ^ 3).  The words of rc(y) are
//           the reverse complements of the words of y, valid together, so staging and
//           extraction are the single-strand ones and the second B operand is made in
//           registers from the same ds_read_b32: with the word right-aligned in 2l bits, its
//           left-aligned reverse complement is pairrev32(w) ^ (~0u << (32 - 2l)) (pairrev32:
//           v_bfrev_b32, then the two bits of every pair swapped), expanded by the routine that
//           expands every other operand.  An invalid word is stored as 0 and its reverse
//           complement is not 0, so that operand takes the forward one's validity handling
//           (empty block skipped, full block as is, mixed block masked).  K2 is symmetric
//           (ham(u, rc(v)) = ham(v, rc(u))) and is half the inner product of the
//           strand-symmetrised feature map c(x) + c(rc(x)); the factor 2 cancels under
//           normalisation, whose diagonals sqrt(K2_ii) carry their own reverse-complement term.
//           Two accumulator sets: per (row, B block) the forward MFMAs go into one v16i and the
//           reverse-complement ones into a second, issued in the order F0 | R0, look up F0,
//           F1, look up R0 | R1, look up F1, ... so that one set's 16 lookups run while the
//           other set's MFMA is in flight.  Both sets' lookups add into one int32 partial (at
//           most 32 adds of <= 12870) before the flush into the lane's int64: the flush rule
//           holds with twice the count.
//   WT      position weights (kmg_gkm_cross_w*, LS-GKM's wgkm): every word carries a weight 0..255
//           that depends on where it starts in its row, and a word pair counts with the product,
//             Kw(x, y) = sum_{a, b} u_x[a] v_y[b] h[ham(x_a, y_b)]   (RC: ... + h[ham(x_a, rc(y_b))])
//           h is not linear in the match count, so the weights cannot go into the one-hot
//           operands: they are applied to the lookups.  GkmxSide.wts holds one byte a word slot
//           in the layout of the words (gkmx_weights_kernel lays the caller's [n][ldw] out); a
//           side without weights (nullptr) is staged as all ones.  The staged chunks bring their
//           weights along (256 B a row and a column), one 16-byte load a thread in the same
//           chunk loops, no extra barrier.
//           In an MFMA result a lane's 16 entries share the B word (lane & 31) and belong to the
//           A words 8 (e / 4) + 4 half + e % 4, so per row of a sweep the lane keeps 16 int32
//           partials T[e] += vB * hm[...] (v_mad_u32_u24; vB one ds_read_u8 a B block; under RC
//           the two sets' lookups are two such multiply-adds with the same vB).  After the
//           column's staged B blocks (at most 8) the partials are flushed, S += sum_e uA[e] T[e]
//           (v_mad_u64_u32; uA the bytes of four aligned dwords of the staged weight row, read
//           once an A block), and start again from 0.  Bounds: T <= 8 * 2 * 255 * 12870 < 2^26;
//           uA * T < 2^34, hence the 64-bit flush; the pair's total is exact in int64 (the API
//           bounds it below 2^53).  An invalid or absent word looks up hm[0] = 0 whatever its
//           weight is, and weight 0 excludes a word.  T costs 16 VGPRs a row, so a WT tile is
//           GX_WTR = 8 rows x 8 columns and a wave owns two rows where the unweighted one owns
//           four: 32 VGPRs of T against 32 fewer of the int64 sums and 16 fewer of A operands,
//           which keeps every instantiation at two waves a SIMD without scratch (the kernel asks
//           for it in its launch bounds).  LDS: 8 KB + 8 KB of words, 2 KB + 2 KB of weights,
//           validity, hm, result: 22 KB.  DIAG: sqrt(Kw(x, x)), both sides staged with x's
//           weights.
//   PF      the mismatch profile (kmg_gkm_profile*, kmg_gkm_cross_f*): N_m = #{(a, b) : ham = m}
//           for m = 0 .. d <= l - 1 instead of sum h[ham].  hm holds a packed counter a bin,
//           hm[mm] = 1 << 8 (m - 4 pass) for the bin m = l - mm of this pass (four bins a pass,
//           ceil((d + 1) / 4) launches), so the same 16 lookups build a histogram: their sum is
//           one int32 of four 8-bit fields (each <= 16, RC <= 32), split by two masks into the
//           pair's two int32 of two 16-bit fields (GxPair; the 64 VGPRs of the int64 sums).  A
//           16-bit field gains at most 8 x 8 blocks x 16 entries x 2 (RC) = 2048 a chunk pair and
//           is flushed once a chunk pair: four xor-shuffle steps packed (16 lanes: 32768), then
//           unpacked to 32 bits for the last two, and lane 0 adds into the pair's int64 bins in
//           LDS (res[16][8][4], 4 KB; only the owning wave writes a pair: no atomics).  hm[0]
//           stays 0, so the bin m = l cannot be counted: it is strands * valid_a * valid_b less
//           the other bins, which the caller can form.  The epilogue stores the pass's bins, or
//           (one pass, d <= 3) applies the caller's real filter c by value,
//           x = ((c[0] N_0 + c[1] N_1) + c[2] N_2) + c[3] N_3 with every product and sum rounded
//           on its own, normalised by one division as above; gkm_filter_kernel applies the same
//           routine to a stored profile for d > 3.  DIAG: the profiles N_m(x, x), or sqrt(x).
//           Not with WT: a weighted field needs 12+ bits an add.  LDS 29.5 KB.
#include "kmg_internal.h"

#include <type_traits>

namespace kmg {

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

constexpr int GX_TR = 16;           // tile rows
constexpr int GX_TC = 8;            // tile columns (and the rows of a DIAG tile)
constexpr int GX_CB = 8;            // 32-word blocks a staged chunk
constexpr int GX_CW = 32 * GX_CB;   // words a staged chunk
constexpr int GX_WTR = 8;           // tile rows of the weighted kernel (WT)

// code and validity of window a of a packed record (pk_window with the validity kept apart)
__device__ __forceinline__ uint32_t gx_window(const uint32_t *rec, int cw, int a, int l, bool &ok) {
  const int i = a >> 4, sh = 2 * (a & 15);
  const uint64_t v = ((uint64_t)rec[i] << 32) | rec[i + 1];
  const int j = a >> 5;
  const uint64_t m = ((((uint64_t)rec[cw + j + 1]) << 32) | rec[cw + j]) >> (a & 31);
  ok = (m & ((1ull << l) - 1ull)) == 0;
  return (uint32_t)((v << sh) >> (64 - 2 * l));
}

// one thread a word slot; a wave covers two 32-word blocks and writes their two validity words
__global__ __launch_bounds__(256) void gkmx_extract_kernel(Packed pk, int64_t n, int l, int pmax,
                                                           int nblk, uint32_t *__restrict__ words,
                                                           uint32_t *__restrict__ bits) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t pp = (int64_t)nblk * 32;
  const bool in = t < n * pp;
  bool ok = false;
  uint32_t code = 0;
  if (in) {
    const int64_t j = t / pp;
    const int a = (int)(t - j * pp);
    if (a < pmax) code = gx_window(pk.w + j * pk.ldp, pk.cw, a, l, ok);
  }
  const uint64_t b = __ballot(ok);
  if (!in) return;
  words[t] = ok ? code : 0u;
  if ((threadIdx.x & 31) == 0) bits[t >> 5] = (uint32_t)(b >> (threadIdx.x & 32));
}

// the caller's weights [n][ldw] -> one byte a word slot, [n][32 nblk], 0 past the row's last
// word; one thread four slots
__global__ __launch_bounds__(256) void gkmx_weights_kernel(const uint8_t *__restrict__ w,
                                                           int64_t ldw,
                                                           const int32_t *__restrict__ lens,
                                                           int64_t n, int l, int nblk,
                                                           uint32_t *__restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x, q = (int64_t)nblk * 8;
  if (t >= n * q) return;
  const int64_t j = t / q;
  const int a = (int)(t - j * q) * 4;
  const int64_t np = min((int64_t)lens[j] - l + 1, ldw);
  uint32_t v = 0u;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (a + i < np) v |= (uint32_t)w[j * ldw + a + i] << (8 * i);
  out[t] = v;
}

template <bool TWO>
struct GxLane {
  uint32_t val[TWO ? 8 : 4];  // 2 where the lane's letter position is < l, else 0
  int lsh, sh0, sh1, lr;      // left-align shift, the two steps' letter-group shifts, word slot
};

// the lane's one-hot dwords of the left-aligned word wl (letter p at bits 31 - 2p, 30 - 2p):
// x0 = MFMA step 0, x1 = step 1
template <bool TWO>
__device__ __forceinline__ void gx_expand_left(const GxLane<TWO> &L, uint32_t wl, v4i &x0, v4i &x1) {
  const uint32_t g0 = wl >> L.sh0;  // the group's 4 letters at bits 7..0 (bits above are masked)
  x0[0] = (int)(L.val[0] << ((g0 >> 3) & 24u));
  x0[1] = (int)(L.val[1] << ((g0 >> 1) & 24u));
  x0[2] = (int)(L.val[2] << ((g0 << 1) & 24u));
  x0[3] = (int)(L.val[3] << ((g0 << 3) & 24u));
  if constexpr (TWO) {
    const uint32_t g1 = wl >> L.sh1;
    x1[0] = (int)(L.val[4] << ((g1 >> 3) & 24u));
    x1[1] = (int)(L.val[5] << ((g1 >> 1) & 24u));
    x1[2] = (int)(L.val[6] << ((g1 << 1) & 24u));
    x1[3] = (int)(L.val[7] << ((g1 << 3) & 24u));
  } else {
    x1 = (v4i){};
  }
}

// ... of the word w as extracted (right-aligned in 2l bits)
template <bool TWO>
__device__ __forceinline__ void gx_expand(const GxLane<TWO> &L, uint32_t w, v4i &x0, v4i &x1) {
  gx_expand_left<TWO>(L, w << L.lsh, x0, x1);
}

// the 16 two-bit pairs of x in reverse order
__device__ __forceinline__ uint32_t gx_pairrev32(uint32_t x) {
  const uint32_t r = __builtin_bitreverse32(x);
  return ((r & 0x55555555u) << 1) | ((r >> 1) & 0x55555555u);
}

template <bool TWO>
__device__ __forceinline__ void gx_mask(const GxLane<TWO> &L, uint32_t vw, v4i &x0, v4i &x1) {
  const int m = -(int)((vw >> L.lr) & 1u);
  x0 &= m;
  if constexpr (TWO) x1 &= m;
}

// one MFMA result: acc[e] = 4 * matches, the byte offset into hm
template <bool TWO>
__device__ __forceinline__ v16i gx_mfma(const v4i &a0, const v4i &a1, const v4i &b0, const v4i &b1) {
  v16i acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0, b0, (v16i){}, 0, 0, 0);
  if constexpr (TWO) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a1, b1, acc, 0, 0, 0);
  return acc;
}

__device__ __forceinline__ int gx_lookup(const int32_t *hm, const v16i &acc) {
  int t = 0;
#pragma unroll
  for (int e = 0; e < 16; ++e) t += *(const int32_t *)((const char *)hm + acc[e]);
  return t;
}

// what a pair's lane adds a looked-up sum t into: the int64 kernel value, or (PF) the profile's
// packed counters.  There the table entry of a match count is 1 << 8 (bin & 3), so t holds four
// 8-bit fields, each <= 16 (RC, both sets added first: <= 32); its even and odd fields go into
// two int32 of two 16-bit fields: q[0] = bins 0 | 2, q[1] = bins 1 | 3 of the pass.
struct GxPair {
  uint32_t q[2];
};
__device__ __forceinline__ void gx_acc(int64_t &S, int t) { S += t; }
__device__ __forceinline__ void gx_acc(GxPair &Q, int t) {
  Q.q[0] += (uint32_t)t & 0x00FF00FFu;
  Q.q[1] += ((uint32_t)t >> 8) & 0x00FF00FFu;
}

// NR rows' operands of one A block against the nbb staged blocks of one column; RC: against
// both strands of the column, two accumulator sets (f forward, g reverse complement)
template <int NR, bool TWO, bool RC, typename ACC>
__device__ __forceinline__ void gx_sweep(const GxLane<TWO> &L, const v4i (&a0)[NR],
                                         const v4i (&a1)[NR], const uint32_t *wcol,
                                         const uint32_t *vcol, int nbb, const int32_t *hm,
                                         ACC (&S)[NR]) {
  for (int bb = 0; bb < nbb; ++bb) {
    const uint32_t vw = __builtin_amdgcn_readfirstlane(vcol[bb]);
    if (vw == 0u) continue;
    v4i b0, b1;
    const uint32_t w = wcol[bb * 32 + L.lr];
    gx_expand<TWO>(L, w, b0, b1);
    if (vw != 0xFFFFFFFFu) gx_mask<TWO>(L, vw, b0, b1);
    if constexpr (!RC) {
#pragma unroll
      for (int r = 0; r < NR; ++r) gx_acc(S[r], gx_lookup(hm, gx_mfma<TWO>(a0[r], a1[r], b0, b1)));
    } else {
      v4i c0, c1;
      gx_expand_left<TWO>(L, gx_pairrev32(w) ^ (0xFFFFFFFFu << L.lsh), c0, c1);
      if (vw != 0xFFFFFFFFu) gx_mask<TWO>(L, vw, c0, c1);
      v16i f = gx_mfma<TWO>(a0[0], a1[0], b0, b1);
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        const v16i g = gx_mfma<TWO>(a0[r], a1[r], c0, c1);  // in flight under f's lookups
        int t = gx_lookup(hm, f);
        if (r + 1 < NR) f = gx_mfma<TWO>(a0[r + 1], a1[r + 1], b0, b1);  // ... under g's
        t += gx_lookup(hm, g);
        gx_acc(S[r], t);  // <= 32 adds of <= 12870 in the int32
      }
    }
  }
}

// WT: the same sweep with the lookups weighted.  ua[r]: the four dwords of row r's staged
// weights that hold the lane's 16 A words; ucol: the column's staged weight bytes.  T <= 8 * 2
// * 255 * 12870 < 2^26 and uA * T < 2^34: the flush is a 64-bit multiply-add.
template <int NR, bool TWO, bool RC>
__device__ __forceinline__ void gx_sweep_w(const GxLane<TWO> &L, const v4i (&a0)[NR],
                                           const v4i (&a1)[NR], const uint32_t (&ua)[NR][4],
                                           const uint32_t *wcol, const uint32_t *vcol,
                                           const uint8_t *ucol, int nbb, const int32_t *hm,
                                           int64_t *S) {
  uint32_t T[NR][16];
#pragma unroll
  for (int r = 0; r < NR; ++r)
#pragma unroll
    for (int e = 0; e < 16; ++e) T[r][e] = 0u;
  auto add = [&](uint32_t (&t)[16], const v16i &acc, uint32_t vB) {
#pragma unroll
    for (int e = 0; e < 16; ++e)
      t[e] += __umul24(vB, (uint32_t) * (const int32_t *)((const char *)hm + acc[e]));
  };
  for (int bb = 0; bb < nbb; ++bb) {
    const uint32_t vw = __builtin_amdgcn_readfirstlane(vcol[bb]);
    if (vw == 0u) continue;
    v4i b0, b1;
    const uint32_t w = wcol[bb * 32 + L.lr];
    const uint32_t vB = ucol[bb * 32 + L.lr];
    gx_expand<TWO>(L, w, b0, b1);
    if (vw != 0xFFFFFFFFu) gx_mask<TWO>(L, vw, b0, b1);
    if constexpr (!RC) {
#pragma unroll
      for (int r = 0; r < NR; ++r) add(T[r], gx_mfma<TWO>(a0[r], a1[r], b0, b1), vB);
    } else {
      v4i c0, c1;
      gx_expand_left<TWO>(L, gx_pairrev32(w) ^ (0xFFFFFFFFu << L.lsh), c0, c1);
      if (vw != 0xFFFFFFFFu) gx_mask<TWO>(L, vw, c0, c1);
      v16i f = gx_mfma<TWO>(a0[0], a1[0], b0, b1);
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        const v16i g = gx_mfma<TWO>(a0[r], a1[r], c0, c1);  // in flight under f's lookups
        add(T[r], f, vB);
        if (r + 1 < NR) f = gx_mfma<TWO>(a0[r + 1], a1[r + 1], b0, b1);  // ... under g's
        add(T[r], g, vB);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    uint64_t acc = (uint64_t)S[r];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      uint32_t u = ua[r][q];
      asm volatile("" : "+v"(u));  // unpack the bytes here, not once for all eight columns
#pragma unroll
      for (int i = 0; i < 4; ++i)
        acc += (uint64_t)((u >> (8 * i)) & 0xFFu) * (uint64_t)T[r][4 * q + i];
    }
    S[r] = (int64_t)acc;
  }
}

// PF: what a profile launch counts and where it goes
struct GxProf {
  int d, pass;    // the bins 4 pass .. 4 pass + 3 of 0 .. d
  int64_t *prof;  // [rows][ldp][d + 1] (DIAG: [n][d + 1]); nullptr: the filter in the epilogue
  int64_t ldp;
  double c[4];    // ... of one pass, d <= 3
};

// x = ((c[0] N_0 + c[1] N_1) + c[2] N_2) + ... up to m = d < NM, every product and sum rounded
// on its own (a float64 host restatement gives the same bits); constant indices into c only
template <int NM>
__device__ __forceinline__ double gx_filter(const double (&c)[NM], const int64_t *N, int d) {
  double x = __dmul_rn(c[0], (double)N[0]);
#pragma unroll
  for (int m = 1; m < NM; ++m)
    if (m <= d) x = __dadd_rn(x, __dmul_rn(c[m], (double)N[m]));
  return x;
}

__device__ __forceinline__ void gx_store(const OutSpec &o, int64_t at, double x, double s) {
  if (o.normalize) x = x / s;
  if (o.dtype == KMG_F64) ((double *)o.out)[at] = x;
  else ((float *)o.out)[at] = (float)x;
}

template <bool DIAG, bool TWO, bool RC, bool WT, bool PF = false>
__global__ __launch_bounds__(256, WT ? 2 : 1) void gram_gkmx_kernel(
    GkmxSide A, GkmxSide B, int l, int64_t row0, int64_t rows, int64_t tiles_c, GkmWeights wt,
    OutSpec o, const double *__restrict__ sa, const double *__restrict__ sb,
    double *__restrict__ dsq_out, GxProf pf) {
  static_assert(!(PF && WT), "a weighted field needs more bits than the profile's registers hold");
  constexpr int TRL = WT ? GX_WTR : GX_TR;            // tile rows the LDS holds
  __shared__ __align__(16) uint32_t wa[TRL][GX_CW];
  __shared__ __align__(16) uint32_t wb[GX_TC][GX_CW];
  __shared__ uint32_t va[TRL][GX_CB], vb[GX_TC][GX_CB];
  __shared__ __align__(16) uint32_t ua[WT ? GX_WTR : 1][GX_CW / 4];  // WT: a weight byte a word
  __shared__ __align__(16) uint32_t ub[WT ? GX_TC : 1][GX_CW / 4];
  __shared__ int32_t hm[20];
  __shared__ int64_t res[GX_TR][GX_TC][PF ? 4 : 1];
  constexpr int TRR = DIAG ? GX_TC : TRL;             // rows a tile
  constexpr int NRW = DIAG ? 1 : TRR / 4;             // rows of one sweep
  constexpr int NCW = DIAG ? 2 : GX_TC;               // sweeps' sums a wave

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int64_t i0, j0;
  int nr, nc;
  if constexpr (DIAG) {
    i0 = j0 = (int64_t)blockIdx.x * GX_TC;
    nr = nc = (int)min((int64_t)GX_TC, A.n - i0);
  } else {
    const int64_t tr = (int64_t)blockIdx.x / tiles_c, tc = (int64_t)blockIdx.x - tr * tiles_c;
    i0 = row0 + tr * TRR;
    j0 = tc * GX_TC;
    nr = (int)min((int64_t)TRR, row0 + rows - i0);
    nc = (int)min((int64_t)GX_TC, B.n - j0);
  }

  if constexpr (PF) {
    // hm[mm] = the counter of the bin m = l - mm where this pass counts it (0 < mm: the bin l of
    // "no match" has no counter, so an all-zero operand still counts nothing), else 0
    if (tid < 20) {
      const int m = l - tid, b = m - 4 * pf.pass;
      hm[tid] = (tid > 0 && m >= 0 && m <= pf.d && b >= 0 && b < 4) ? 1 << (8 * b) : 0;
    }
    for (int t = tid; t < GX_TR * GX_TC * 4; t += 256) (&res[0][0][0])[t] = 0;
  } else {
    // hm[m] = h[l - m] (constant indices into wt only: it stays in scalar registers)
#pragma unroll
    for (int d = 0; d < 17; ++d)
      if (tid == l - d) hm[tid] = wt.h[d];
    if (tid > l && tid < 20) hm[tid] = 0;
  }

  GxLane<TWO> L;
  L.lr = lane & 31;
  const int half = lane >> 5;
  L.lsh = 32 - 2 * l;
  L.sh0 = 24 - 8 * half;
  L.sh1 = 8 - 8 * half;
#pragma unroll
  for (int q = 0; q < (TWO ? 8 : 4); ++q) L.val[q] = (8 * (q >> 2) + 4 * half + (q & 3)) < l ? 2u : 0u;

  typename std::conditional<PF, GxPair, int64_t>::type S[NCW][NRW];  // 64 VGPRs either way
#pragma unroll
  for (int c = 0; c < NCW; ++c)
#pragma unroll
    for (int r = 0; r < NRW; ++r) S[c][r] = {};

  const int nca = (A.nblk + GX_CB - 1) / GX_CB, ncb = (B.nblk + GX_CB - 1) / GX_CB;
  for (int ca = 0; ca < nca; ++ca) {
    for (int cb = 0; cb < ncb; ++cb) {
      __syncthreads();  // the previous chunk's sweeps are done (and hm is written)
      if (cb == 0) {
        for (int t = tid; t < TRR * (GX_CW / 4); t += 256) {
          const int r = t / (GX_CW / 4), q4 = (t % (GX_CW / 4)) * 4, blk = ca * GX_CB + (q4 >> 5);
          uint4 v = make_uint4(0u, 0u, 0u, 0u);
          if (r < nr && blk < A.nblk)
            v = *(const uint4 *)(A.words + ((i0 + r) * A.nblk + blk) * 32 + (q4 & 31));
          *(uint4 *)&wa[r][q4] = v;
        }
        if (tid < TRR * GX_CB) {
          const int r = tid / GX_CB, blk = ca * GX_CB + tid % GX_CB;
          va[r][tid % GX_CB] = (r < nr && blk < A.nblk) ? A.bits[(i0 + r) * A.nblk + blk] : 0u;
        }
        if constexpr (WT) {
          if (tid < TRR * (GX_CW / 16)) {
            const int r = tid / (GX_CW / 16), q16 = (tid % (GX_CW / 16)) * 16;
            const int blk = ca * GX_CB + (q16 >> 5);
            uint4 v = make_uint4(0x01010101u, 0x01010101u, 0x01010101u, 0x01010101u);
            if (A.wts) {
              v = make_uint4(0u, 0u, 0u, 0u);
              if (r < nr && blk < A.nblk)
                v = *(const uint4 *)(A.wts + ((i0 + r) * A.nblk + blk) * 32 + (q16 & 31));
            }
            *(uint4 *)&ua[r][q16 / 4] = v;
          }
        }
      }
      for (int t = tid; t < GX_TC * (GX_CW / 4); t += 256) {
        const int r = t / (GX_CW / 4), q4 = (t % (GX_CW / 4)) * 4, blk = cb * GX_CB + (q4 >> 5);
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (r < nc && blk < B.nblk)
          v = *(const uint4 *)(B.words + ((j0 + r) * B.nblk + blk) * 32 + (q4 & 31));
        *(uint4 *)&wb[r][q4] = v;
      }
      if (tid < GX_TC * GX_CB) {
        const int r = tid / GX_CB, blk = cb * GX_CB + tid % GX_CB;
        vb[r][tid % GX_CB] = (r < nc && blk < B.nblk) ? B.bits[(j0 + r) * B.nblk + blk] : 0u;
      }
      if constexpr (WT) {
        if (tid >= 128) {  // (the first two waves have staged the validity words)
          const int t = tid - 128, r = t / (GX_CW / 16), q16 = (t % (GX_CW / 16)) * 16;
          const int blk = cb * GX_CB + (q16 >> 5);
          uint4 v = make_uint4(0x01010101u, 0x01010101u, 0x01010101u, 0x01010101u);
          if (B.wts) {
            v = make_uint4(0u, 0u, 0u, 0u);
            if (r < nc && blk < B.nblk)
              v = *(const uint4 *)(B.wts + ((j0 + r) * B.nblk + blk) * 32 + (q16 & 31));
          }
          *(uint4 *)&ub[r][q16 / 4] = v;
        }
      }
      __syncthreads();

      const int nba = min(GX_CB, A.nblk - ca * GX_CB), nbb = min(GX_CB, B.nblk - cb * GX_CB);
      if constexpr (DIAG) {
#pragma unroll
        for (int rr = 0; rr < 2; ++rr) {
          const int r = 2 * wave + rr;
          if (r >= nr) continue;  // wave-uniform
          for (int ab = 0; ab < nba; ++ab) {
            const uint32_t vw = __builtin_amdgcn_readfirstlane(va[r][ab]);
            if (vw == 0u) continue;
            v4i a0[1], a1[1];
            gx_expand<TWO>(L, wa[r][ab * 32 + L.lr], a0[0], a1[0]);
            gx_mask<TWO>(L, vw, a0[0], a1[0]);
            if constexpr (WT) {
              uint32_t u[1][4];
#pragma unroll
              for (int q = 0; q < 4; ++q) u[0][q] = ua[r][ab * 8 + 2 * q + half];
              gx_sweep_w<1, TWO, RC>(L, a0, a1, u, wb[r], vb[r], (const uint8_t *)ub[r], nbb, hm,
                                     S[rr]);
            } else {
              gx_sweep<1, TWO, RC>(L, a0, a1, wb[r], vb[r], nbb, hm, S[rr]);
            }
          }
        }
      } else if constexpr (WT) {
        const int rb = NRW * wave;
        if (rb < nr) {  // wave-uniform
          for (int ab = 0; ab < nba; ++ab) {
            v4i a0[NRW], a1[NRW];
            uint32_t u[NRW][4];
            uint32_t any = 0u;
#pragma unroll
            for (int r = 0; r < NRW; ++r) {
              const uint32_t vw = va[rb + r][ab];
              any |= vw;
              gx_expand<TWO>(L, wa[rb + r][ab * 32 + L.lr], a0[r], a1[r]);
              gx_mask<TWO>(L, vw, a0[r], a1[r]);
#pragma unroll
              for (int q = 0; q < 4; ++q) u[r][q] = ua[rb + r][ab * 8 + 2 * q + half];
            }
            if (__builtin_amdgcn_readfirstlane(any) == 0u) continue;
#pragma unroll
            for (int c = 0; c < GX_TC; ++c)
              if (c < nc)
                gx_sweep_w<NRW, TWO, RC>(L, a0, a1, u, wb[c], vb[c], (const uint8_t *)ub[c], nbb,
                                         hm, S[c]);
          }
        }
      } else {
        const int rb = 4 * wave;
        if (rb < nr) {  // wave-uniform
          for (int ab = 0; ab < nba; ++ab) {
            v4i a0[4], a1[4];
            uint32_t any = 0u;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const uint32_t vw = va[rb + r][ab];
              any |= vw;
              gx_expand<TWO>(L, wa[rb + r][ab * 32 + L.lr], a0[r], a1[r]);
              gx_mask<TWO>(L, vw, a0[r], a1[r]);
            }
            if (__builtin_amdgcn_readfirstlane(any) == 0u) continue;
#pragma unroll
            for (int c = 0; c < GX_TC; ++c)
              if (c < nc) gx_sweep<4, TWO, RC>(L, a0, a1, wb[c], vb[c], nbb, hm, S[c]);
          }
        }
      }
      if constexpr (PF) {
        // the flush, once a chunk pair.  A lane's 16-bit field has gained at most GX_CB * GX_CB
        // blocks * 16 entries * 2 (RC) = 2048 since the last one, so four xor-shuffle steps still
        // fit it (16 lanes: 32768); then the fields are unpacked to 32 bits for the last two
        // steps and lane 0 adds them to the pair's int64 bins.  Only the owning wave touches a
        // pair's bins, so this needs neither atomics nor a barrier.
        static_assert(GX_CB * GX_CB * 16 * 2 * 16 <= 65535, "a packed field overflows in the flush");
        if ((DIAG ? 2 : NRW) * wave < nr) {  // wave-uniform
#pragma unroll
          for (int c = 0; c < NCW; ++c)
#pragma unroll
            for (int r = 0; r < NRW; ++r) {
              uint32_t q0 = S[c][r].q[0], q1 = S[c][r].q[1];
              S[c][r] = {};
#pragma unroll
              for (int d = 1; d <= 8; d <<= 1) {
                q0 += __shfl_xor(q0, d, 64);
                q1 += __shfl_xor(q1, d, 64);
              }
              uint32_t n[4] = {q0 & 0xFFFFu, q1 & 0xFFFFu, q0 >> 16, q1 >> 16};
#pragma unroll
              for (int b = 0; b < 4; ++b) {
                n[b] += __shfl_xor(n[b], 16, 64);
                n[b] += __shfl_xor(n[b], 32, 64);
              }
              if (lane == 0) {
                int64_t *bins = DIAG ? res[2 * wave + c][0] : res[NRW * wave + r][c];
#pragma unroll
                for (int b = 0; b < 4; ++b) bins[b] += n[b];
              }
            }
        }
      }
    }
  }

  // one cross-lane reduction a pair
  if constexpr (!PF) {
#pragma unroll
    for (int c = 0; c < NCW; ++c)
#pragma unroll
      for (int r = 0; r < NRW; ++r) {
        int64_t v = S[c][r];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
        if (lane == 0) {
          if constexpr (DIAG) res[2 * wave + c][0][0] = v;
          else res[NRW * wave + r][c][0] = v;
        }
      }
  }
  __syncthreads();

  if constexpr (PF) {
    // the pass's bins into the stored profile, or (one pass, d <= 3) the filtered value
    const int r = DIAG ? tid : tid / GX_TC, c = DIAG ? 0 : tid % GX_TC;
    if (tid >= GX_TR * GX_TC || r >= nr || c >= nc) return;
    const int64_t *N = res[r][c];
    const int64_t at = DIAG ? i0 + r : (i0 - row0 + r) * (pf.prof ? pf.ldp : o.ld) + j0 + c;
    if (pf.prof) {
#pragma unroll
      for (int b = 0; b < 4; ++b)
        if (4 * pf.pass + b <= pf.d) pf.prof[at * (pf.d + 1) + 4 * pf.pass + b] = N[b];
    } else {
      const double x = gx_filter<4>(pf.c, N, pf.d);
      if constexpr (DIAG) dsq_out[at] = __builtin_sqrt(x);
      else gx_store(o, at, x, o.normalize ? sa[i0 + r] * sb[j0 + c] : 1.0);
    }
    return;
  }

  if constexpr (DIAG) {
    if (tid < nr) dsq_out[i0 + tid] = __builtin_sqrt((double)res[tid][0][0]);  // IEEE sqrt (RC: K2_ii)
  } else {
    const int r = tid / GX_TC, c = tid % GX_TC;
    if (tid < GX_TR * GX_TC && r < nr && c < nc) {
      const int64_t v = res[r][c][0];
      const int64_t at = (i0 - row0 + r) * o.ld + j0 + c;
      if (o.dtype == KMG_I32) {
        ((int32_t *)o.out)[at] = (int32_t)v;
      } else {
        const double x = o.normalize ? (double)v / (sa[i0 + r] * sb[j0 + c]) : (double)v;
        if (o.dtype == KMG_F64) ((double *)o.out)[at] = x;
        else ((float *)o.out)[at] = (float)x;
      }
    }
  }
}

// the instantiation of a launch: two MFMA steps (l > 8), both strands, position weights
template <bool DIAG>
auto gx_kernel(bool two, bool rc, bool wt) {
  decltype(&gram_gkmx_kernel<DIAG, false, false, false>) k[8] = {
      gram_gkmx_kernel<DIAG, false, false, false>, gram_gkmx_kernel<DIAG, false, false, true>,
      gram_gkmx_kernel<DIAG, false, true, false>,  gram_gkmx_kernel<DIAG, false, true, true>,
      gram_gkmx_kernel<DIAG, true, false, false>,  gram_gkmx_kernel<DIAG, true, false, true>,
      gram_gkmx_kernel<DIAG, true, true, false>,   gram_gkmx_kernel<DIAG, true, true, true>};
  return k[4 * two + 2 * rc + wt];
}

// ... of a profile launch (PF)
template <bool DIAG>
auto gx_kernel_pf(bool two, bool rc) {
  decltype(&gram_gkmx_kernel<DIAG, false, false, false, true>) k[4] = {
      gram_gkmx_kernel<DIAG, false, false, false, true>, gram_gkmx_kernel<DIAG, false, true, false, true>,
      gram_gkmx_kernel<DIAG, true, false, false, true>,  gram_gkmx_kernel<DIAG, true, true, false, true>};
  return k[2 * two + rc];
}

// sum_m c[m] N_m over a stored profile, one thread a pair
__global__ __launch_bounds__(256) void gkm_filter_kernel(const int64_t *__restrict__ prof,
                                                         int64_t rows, int64_t cols, int64_t ldp,
                                                         int d, GkmFilter f, OutSpec o,
                                                         const double *__restrict__ sa,
                                                         const double *__restrict__ sb,
                                                         double *__restrict__ dsq_out) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= rows * cols) return;
  const int64_t i = t / cols, j = t - i * cols;
  const double x = gx_filter<16>(f.c, prof + (i * ldp + j) * (d + 1), d);
  if (dsq_out) dsq_out[i] = __builtin_sqrt(x);
  else gx_store(o, i * o.ld + j, x, o.normalize ? sa[i] * sb[j] : 1.0);
}

// the passes of a profile launch (prof) or the one pass of a filtered one (f), rows split so
// every launch stays below KMG_GKM_MAX_TILES tiles
hipError_t gx_launch_pf(const GkmxSide &A, const GkmxSide &B, int l, int d, bool rc, int64_t row0,
                        int64_t rows, int64_t *prof, int64_t ldp, const GkmFilter *f,
                        const OutSpec &o, const double *sa, const double *sb, hipStream_t s) {
  if (rows <= 0 || B.n <= 0) return hipSuccess;
  if (l < 1 || l > 16 || d < 0 || d > l - 1 || A.nblk < 1 || B.nblk < 1 || A.wts || B.wts ||
      row0 < 0 || row0 + rows > A.n)
    return hipErrorInvalidValue;
  if (prof ? ldp < B.n : (d > 3 || !o.out || o.ld < B.n || (o.normalize && (!sa || !sb))))
    return hipErrorInvalidValue;
  const int64_t tiles_c = (B.n + GX_TC - 1) / GX_TC;
  if (tiles_c >= KMG_GKM_MAX_TILES) return hipErrorInvalidValue;  // AQL grid size is 32-bit
  const int64_t max_rows = (KMG_GKM_MAX_TILES - 1) / tiles_c * GX_TR;
  const size_t esz = o.dtype == KMG_F64 ? 8 : 4;
  const auto kern = gx_kernel_pf<false>(l > 8, rc);
  for (int pass = 0; 4 * pass <= d; ++pass)
    for (int64_t r0 = 0; r0 < rows; r0 += max_rows) {
      const int64_t nr = rows - r0 < max_rows ? rows - r0 : max_rows;
      GxProf pf{d, pass, prof ? prof + r0 * ldp * (d + 1) : nullptr, ldp, {}};
      for (int m = 0; f && m <= d; ++m) pf.c[m] = f->c[m];
      OutSpec os = o;
      if (!prof) os.out = (char *)o.out + (size_t)r0 * o.ld * esz;
      hipLaunchKernelGGL(kern, dim3((unsigned)((nr + GX_TR - 1) / GX_TR * tiles_c)), dim3(256), 0, s,
                         A, B, l, row0 + r0, nr, tiles_c, GkmWeights{}, os, sa, sb,
                         (double *)nullptr, pf);
      const hipError_t e = hipGetLastError();
      if (e != hipSuccess) return e;
    }
  return hipSuccess;
}

hipError_t gx_launch_pf_diag(const GkmxSide &A, int l, int d, bool rc, int64_t *prof,
                             const GkmFilter *f, double *dsq, hipStream_t s) {
  if (A.n <= 0) return hipSuccess;
  if (l < 1 || l > 16 || d < 0 || d > l - 1 || A.nblk < 1 || A.wts) return hipErrorInvalidValue;
  if (prof ? false : (d > 3 || !f || !dsq)) return hipErrorInvalidValue;
  const int64_t tiles = (A.n + GX_TC - 1) / GX_TC;
  if (tiles >= KMG_GKM_MAX_TILES) return hipErrorInvalidValue;
  const auto kern = gx_kernel_pf<true>(l > 8, rc);
  for (int pass = 0; 4 * pass <= d; ++pass) {
    GxProf pf{d, pass, prof, 1, {}};
    for (int m = 0; f && m <= d; ++m) pf.c[m] = f->c[m];
    hipLaunchKernelGGL(kern, dim3((unsigned)tiles), dim3(256), 0, s, A, A, l, (int64_t)0, A.n,
                       (int64_t)1, GkmWeights{}, OutSpec{}, (const double *)nullptr,
                       (const double *)nullptr, dsq, pf);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace

hipError_t launch_gkmx_profile(const GkmxSide &A, const GkmxSide &B, int l, int d, bool rc,
                               int64_t row0, int64_t rows, int64_t *prof, int64_t ldp,
                               hipStream_t s) {
  if (!prof) return hipErrorInvalidValue;
  return gx_launch_pf(A, B, l, d, rc, row0, rows, prof, ldp, nullptr, OutSpec{}, nullptr, nullptr, s);
}

hipError_t launch_gkmx_profile_diag(const GkmxSide &A, int l, int d, bool rc, int64_t *prof,
                                    hipStream_t s) {
  if (!prof) return hipErrorInvalidValue;
  return gx_launch_pf_diag(A, l, d, rc, prof, nullptr, nullptr, s);
}

hipError_t launch_gkmx_filtered(const GkmxSide &A, const GkmxSide &B, int l, int d, bool rc,
                                const GkmFilter &f, const OutSpec &o, const double *sa,
                                const double *sb, hipStream_t s) {
  return gx_launch_pf(A, B, l, d, rc, 0, A.n, nullptr, 0, &f, o, sa, sb, s);
}

hipError_t launch_gkmx_filtered_diag(const GkmxSide &A, int l, int d, bool rc, const GkmFilter &f,
                                     double *dsq, hipStream_t s) {
  return gx_launch_pf_diag(A, l, d, rc, nullptr, &f, dsq, s);
}

hipError_t launch_gkm_filter(const int64_t *prof, int64_t rows, int64_t cols, int64_t ldp, int d,
                             const GkmFilter &f, const OutSpec &o, const double *sa,
                             const double *sb, double *dsq, hipStream_t s) {
  if (rows <= 0 || cols <= 0) return hipSuccess;
  if (!prof || d < 0 || d > 15 || ldp < cols) return hipErrorInvalidValue;
  if (dsq ? cols != 1 : (!o.out || o.ld < cols || (o.normalize && (!sa || !sb))))
    return hipErrorInvalidValue;
  const int64_t blocks = (rows * cols + 255) / 256;
  if (blocks >= ((int64_t)1 << 31)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gkm_filter_kernel, dim3((unsigned)blocks), dim3(256), 0, s, prof, rows, cols,
                     ldp, d, f, o, sa, sb, dsq);
  return hipGetLastError();
}

hipError_t launch_gkmx_weights(const uint8_t *w, int64_t ldw, const int32_t *lens, int64_t n, int l,
                               int pmax, uint8_t *out, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  if (pmax < 1 || l < 1 || l > 16 || ldw < 0 || !w || !lens || !out) return hipErrorInvalidValue;
  const int nblk = gkmx_blocks(pmax);
  const int64_t blocks = (n * nblk * 8 + 255) / 256;
  if (blocks >= KMG_GKM_MAX_TILES) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gkmx_weights_kernel, dim3((unsigned)blocks), dim3(256), 0, s, w, ldw, lens, n,
                     l, nblk, (uint32_t *)out);
  return hipGetLastError();
}

hipError_t launch_gkmx_extract(const Packed &pk, int64_t n, int l, int pmax, uint32_t *words,
                               uint32_t *bits, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  if (pmax < 1 || l < 1 || l > 16) return hipErrorInvalidValue;
  const int nblk = gkmx_blocks(pmax);
  const int64_t blocks = (n * nblk * 32 + 255) / 256;
  if (blocks >= KMG_GKM_MAX_TILES) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gkmx_extract_kernel, dim3((unsigned)blocks), dim3(256), 0, s, pk, n, l, pmax,
                     nblk, words, bits);
  return hipGetLastError();
}

hipError_t launch_gram_gkmx(const GkmxSide &A, const GkmxSide &B, int l, bool rc,
                            const GkmWeights &wt, const OutSpec &o, const double *sa,
                            const double *sb, hipStream_t s) {
  if (A.n <= 0 || B.n <= 0) return hipSuccess;
  if (l < 1 || l > 16 || A.nblk < 1 || B.nblk < 1) return hipErrorInvalidValue;
  if (o.normalize && (!sa || !sb)) return hipErrorInvalidValue;
  const int64_t tiles_c = (B.n + GX_TC - 1) / GX_TC;
  if (tiles_c >= KMG_GKM_MAX_TILES) return hipErrorInvalidValue;  // AQL grid size is 32-bit
  const bool wts = A.wts || B.wts;
  const int tr = wts ? GX_WTR : GX_TR;
  const int64_t max_rows = (KMG_GKM_MAX_TILES - 1) / tiles_c * tr;
  const size_t esz = o.dtype == KMG_F64 ? 8 : 4;
  const auto kern = gx_kernel<false>(l > 8, rc, wts);
  for (int64_t r0 = 0; r0 < A.n; r0 += max_rows) {
    const int64_t rows = A.n - r0 < max_rows ? A.n - r0 : max_rows;
    const dim3 grid((unsigned)((rows + tr - 1) / tr * tiles_c));
    OutSpec os = o;
    os.out = (char *)o.out + (size_t)r0 * o.ld * esz;
    hipLaunchKernelGGL(kern, grid, dim3(256), 0, s, A, B, l, r0, rows, tiles_c, wt, os, sa, sb,
                       (double *)nullptr, GxProf{});
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_gkmx_diag(const GkmxSide &A, int l, bool rc, const GkmWeights &wt, double *dsq,
                            hipStream_t s) {
  if (A.n <= 0) return hipSuccess;
  if (l < 1 || l > 16 || A.nblk < 1) return hipErrorInvalidValue;
  const int64_t tiles = (A.n + GX_TC - 1) / GX_TC;
  if (tiles >= KMG_GKM_MAX_TILES) return hipErrorInvalidValue;
  const OutSpec o{};
  const auto kern = gx_kernel<true>(l > 8, rc, A.wts != nullptr);
  hipLaunchKernelGGL(kern, dim3((unsigned)tiles), dim3(256), 0, s, A, A, l, (int64_t)0, A.n,
                     (int64_t)1, wt, o, (const double *)nullptr, (const double *)nullptr, dsq,
                     GxProf{});
  return hipGetLastError();
}

}  // namespace kmg
