/*
 * sdrfm_loudness.h — the stereo PCM sink's per-stream K-weighted loudness meter (include/sdrfm.h): the one copy of the
 * K-weighting step, of the index arithmetic and of the matrix-power table that the kernel, the plain-C host side (csrc/loudness.c), the sink's
 * host code and the CPU checks all use, and the kernel's body.
 *
 * K-weighting is two cascaded biquads per channel, a recursion along the row.  It is linear: the filter state after a chunk is
 * A^len · (state before) + (state the chunk leaves from zero), A the 4 x 4 zero-input transition of the cascade.  So a tile of SDRFM_LD_TILE
 * pairs is cut into SDRFM_LD_NT chunks of SDRFM_LD_L pairs, one per lane: pass 1 runs every chunk from zero state (lane 0 from the carried
 * state), a Hillis-Steele scan over lanes with the precomputed powers A^(L·2^i), in coordinates that keep those powers' entries below 1
 * (ld_balance), gives every lane its true incoming state, pass 2 runs the chunk again from that state and sums y^2.  With block_len >= 64 >= L a chunk touches at most two sub-blocks: a lane leaves two partial sums
 * per channel and a split point, and one lane per sub-block and channel adds the pieces in lane order.  No atomics, one fixed order.
 *
 * The first part is plain C99, no HIP types: csrc/loudness.c, tests/native/loudness_check.cpp and tools/loudness_emulate.py's checks compile or
 * restate it with a host compiler alone.  The kernel's body follows under __HIPCC__.  Internal to the library; the boundary is include/sdrfm.h.
 */
#ifndef SDRFM_LOUDNESS_H
#define SDRFM_LOUDNESS_H

#include <stdint.h>

#include "../../include/sdrfm.h"

#if defined(__HIPCC__)
#define SDRFM_LD_FN __host__ __device__ __forceinline__
#else
#define SDRFM_LD_FN static inline
#endif

/* the geometry.  L is odd so that lane-per-chunk LDS reads (a stride of L dwords) fall on distinct banks; 256 x 19 = 4864 covers the
 * 4800-pair call of a tenth of a second in one tile.  SDRFM_LD_L_CHECK lets a CPU check shrink the tile; the library never defines it. */
#ifdef SDRFM_LD_L_CHECK
#define SDRFM_LD_L SDRFM_LD_L_CHECK
#define SDRFM_LD_NT SDRFM_LD_NT_CHECK
#else
#define SDRFM_LD_L 19u                              /* pairs per lane */
#define SDRFM_LD_NT 256u                            /* lanes of a stream's workgroup: four waves */
#endif
#define SDRFM_LD_TILE (SDRFM_LD_NT * SDRFM_LD_L)    /* pairs per tile */
#define SDRFM_LD_STEPS 8u                           /* powers A^(L 2^i), i < 8: a scan over up to 256 lanes */
#define SDRFM_LD_TABLE (SDRFM_LD_STEPS * 16u + 2u)   /* doubles of the device table: the powers, then kappa and 1 / kappa */
#define SDRFM_LD_BLOCK_MIN 64u
#define SDRFM_LD_BLOCK_MAX (1u << 20)
#define SDRFM_LD_CAP_MAX 4096u

/* ---- the K-weighting step: both biquads in transposed direct form II, z = {shelf s1, shelf s2, high-pass s1, high-pass s2}.  Every product
 * and every sum is rounded on its own (the library and loudness.o are built with -ffp-contract=off); the order is the definition ---------- */
SDRFM_LD_FN double ld_kw_step(const double* c, double* z, double x) {
  const double y1 = c[0] * x + z[0];
  z[0] = (c[1] * x - c[3] * y1) + z[1];
  z[1] = c[2] * x - c[4] * y1;
  const double y2 = c[5] * y1 + z[2];
  z[2] = (c[6] * y1 - c[8] * y2) + z[3];
  z[3] = c[7] * y1 - c[9] * y2;
  return y2;
}

/* the zero-input transition of ld_kw_step, row-major: z' = A z */
SDRFM_LD_FN void ld_transition(const double* c, double* A) {
  for (int k = 0; k < 16; ++k) A[k] = 0.0;
  A[0] = -c[3];  A[1] = 1.0;                        /* shelf s1' = -a1 s1 + s2 */
  A[4] = -c[4];                                     /* shelf s2' = -a2 s1 */
  A[8] = c[6] - c[8] * c[5];  A[10] = -c[8];  A[11] = 1.0;   /* y1 = s1a, y2 = b0 y1 + s1b */
  A[12] = c[7] - c[9] * c[5]; A[14] = -c[9];
}

/* kappa, a power of two in 1 .. 2^20: the scan runs in the coordinates (z0, z1, z2, kappa (z2 + z3)) per channel.  The high-pass's poles lie at
 * radius 0.995 a few milliradians from z = 1; in its own transposed-form coordinates the powers of its transition grow to about 75 before they
 * decay, and a product with a state of 5e4 LSB rounds at 75 x 5e4 ulp, which the recursion then amplifies again.  With the second coordinate
 * replaced by the SUM of the two states (small when the input moves slowly; the sum of two close doubles is exact) and scaled by
 * kappa ~ 1 / sqrt(1 + a1 + a2), the transition is close to a rotation and no entry of any power exceeds 1.  A power of two scales exactly */
SDRFM_LD_FN double ld_balance(const double* c) {
  const double t = 1.0 + c[8] + c[9];                /* > 0 for poles inside the unit circle */
  double kappa = 1.0;
  for (int k = 0; k < 20 && 2.0 * kappa * kappa * t < 1.0; ++k) kappa = kappa * 2.0;   /* stop where kappa^2 t is nearest 1 on a log scale */
  return kappa;
}

/* pw[i] = (T A T^-1)^(L 2^i), i < SDRFM_LD_STEPS, T z = (z0, z1, z2, kappa (z2 + z3)): the transition taken into the scan's coordinates first,
 * where its powers are products without cancellation, then its L-th power by L - 1 products from the left, then repeated squaring, all in
 * LONG DOUBLE and rounded to double at the end; then kappa and 1 / kappa.  Host only.  A power evaluated in double, or in the filter's own
 * coordinates, is off by many ulp, which the scan would multiply into every state: the table is where the kernel's precision is decided */
static inline void ld_matmul_l(const long double* X, const long double* Y, long double* out) {   /* out = X Y, out distinct from both */
  for (int r = 0; r < 4; ++r)
    for (int q = 0; q < 4; ++q) {
      long double t = X[4 * r] * Y[q];
      for (int k = 1; k < 4; ++k) t = t + X[4 * r + k] * Y[4 * k + q];
      out[4 * r + q] = t;
    }
}

static inline void ld_matrix_powers(const double* c, double* pw /* [SDRFM_LD_TABLE] */) {
  double Ad[16];
  long double A[16], P[16], t[16], u[16], T[16], Ti[16];
  const long double kappa = (long double)ld_balance(c);
  ld_transition(c, Ad);
  for (int k = 0; k < 16; ++k) {
    u[k] = (long double)Ad[k];
    T[k] = Ti[k] = (k % 5 == 0) ? 1.0L : 0.0L;
  }
  T[14] = T[15] = kappa;
  Ti[14] = -1.0L;
  Ti[15] = 1.0L / kappa;
  ld_matmul_l(T, u, t);
  ld_matmul_l(t, Ti, A);
  for (int k = 0; k < 16; ++k) P[k] = A[k];
  for (uint32_t j = 1; j < SDRFM_LD_L; ++j) {
    ld_matmul_l(A, P, t);
    for (int k = 0; k < 16; ++k) P[k] = t[k];
  }
  for (uint32_t i = 0; i < SDRFM_LD_STEPS; ++i) {
    for (int k = 0; k < 16; ++k) pw[16 * i + k] = (double)P[k];
    ld_matmul_l(P, P, t);
    for (int k = 0; k < 16; ++k) P[k] = t[k];
  }
  pw[16 * SDRFM_LD_STEPS] = (double)kappa;
  pw[16 * SDRFM_LD_STEPS + 1] = (double)(1.0L / kappa);
}

/* p += M q, the scan's combine: a row's products added left to right, then the row onto p */
SDRFM_LD_FN void ld_matvec_add(const double* M, const double* q, double* p) {
  for (int r = 0; r < 4; ++r) {
    double t = M[4 * r] * q[0];
    t = t + M[4 * r + 1] * q[1];
    t = t + M[4 * r + 2] * q[2];
    t = t + M[4 * r + 3] * q[3];
    p[r] = p[r] + t;
  }
}

/* ---- index arithmetic, plain integers ------------------------------------------------------------------------------------------------------ */
SDRFM_LD_FN uint32_t ld_tiles(uint32_t n) { return (uint32_t)(((uint64_t)n + SDRFM_LD_TILE - 1u) / SDRFM_LD_TILE); }

/* the pairs of tile t of a call of n */
SDRFM_LD_FN uint32_t ld_tile_len(uint32_t n, uint32_t t) {
  const uint64_t left = (uint64_t)n - (uint64_t)t * SDRFM_LD_TILE;
  return left < SDRFM_LD_TILE ? (uint32_t)left : SDRFM_LD_TILE;
}

/* the lanes of a tile of m pairs that have a chunk */
SDRFM_LD_FN uint32_t ld_active_lanes(uint32_t m) { return (m + SDRFM_LD_L - 1u) / SDRFM_LD_L; }

/* the chunk of `lane` in a tile of m pairs: pairs begin .. begin + len of the tile, len = 0 for a lane behind the tile's end */
SDRFM_LD_FN void ld_chunk(uint32_t m, uint32_t lane, uint32_t* begin, uint32_t* len) {
  const uint32_t b = lane * SDRFM_LD_L;
  *begin = b < m ? b : m;
  *len = b >= m ? 0u : (m - b < SDRFM_LD_L ? m - b : SDRFM_LD_L);
}

/* a chunk of len pairs that starts `off` pairs into its sub-block (off < block_len): how many of its pairs lie in that sub-block; the
 * others lie in the next one, and in no third because len <= L <= 64 <= block_len */
SDRFM_LD_FN uint32_t ld_split(uint32_t off, uint32_t block_len, uint32_t len) {
  const uint32_t room = block_len - off;
  return len < room ? len : room;
}

/* a tile of m pairs that starts `off` pairs into a sub-block: the sub-blocks it completes, and where the next tile starts in its own */
SDRFM_LD_FN uint32_t ld_tile_blocks(uint32_t off, uint32_t m, uint32_t block_len) { return (off + m) / block_len; }
SDRFM_LD_FN uint32_t ld_tile_next_off(uint32_t off, uint32_t m, uint32_t block_len) { return (off + m) % block_len; }

/* sub-block k of such a tile (k = 0 is the one the tile starts in, k = ld_tile_blocks is the one it leaves open): the tile's pairs lo .. hi
 * that lie in it (hi <= lo: none), and *start = where it begins relative to the tile, negative when it began before the tile */
SDRFM_LD_FN void ld_block_span(uint32_t off, uint32_t m, uint32_t block_len, uint32_t k, int64_t* start, uint32_t* lo, uint32_t* hi) {
  const int64_t bs = (int64_t)k * (int64_t)block_len - (int64_t)off;
  const int64_t be = bs + (int64_t)block_len;
  *start = bs;
  *lo = bs < 0 ? 0u : (bs < (int64_t)m ? (uint32_t)bs : m);
  *hi = be < (int64_t)m ? (uint32_t)be : m;
}

/* of a lane whose chunk meets sub-block k: 0 when its pairs in k are the chunk's first part, 1 when they are the second */
SDRFM_LD_FN uint32_t ld_piece(uint32_t lane, int64_t start) { return (int64_t)(lane * SDRFM_LD_L) >= start ? 0u : 1u; }

/* a call of n pairs on a stream that has consumed pos: the sub-blocks it completes */
SDRFM_LD_FN uint64_t ld_blocks_done(uint64_t pos, uint32_t n, uint32_t block_len) { return (pos + n) / block_len - pos / block_len; }

/* the ring: sub-block b lives in slot b % cap, and of `total` completed sub-blocks only those from ld_keep_from on are stored, so that a
 * call which completes more than cap writes each slot once */
SDRFM_LD_FN uint32_t ld_ring_slot(uint64_t b, uint32_t cap) { return (uint32_t)(b % cap); }
SDRFM_LD_FN uint64_t ld_keep_from(uint64_t total, uint32_t cap) { return total > cap ? total - cap : 0u; }

/* ---- the domain: the coefficient sets the device may be enabled with.  Host only ------------------------------------------------------------
 * The scan is exact in exact arithmetic for every stable set; what it loses to rounding depends on the set, and neither kappa, nor the largest
 * entry of the table, nor the pole radii bound it: the 96 kHz K-weighting and the 48 kHz shelf over a high-pass with the same poles lie a
 * factor of nine apart.  So the predicate measures.  ld_emulate_channel is the kernel's order of operations for one channel
 * in plain C — what tools/loudness_emulate.py restates in numpy —, ld_reference_channel the definition, and ld_probe runs both over the rows on
 * which the difference peaks: DC at the positive rail in calls of 4800 and 4800 pairs and in one of 2 TILE + 17, DC and a full-range burst of
 * 4800 pairs each followed by three calls of zeros, a full-range row of TILE + 1; at block_len 64 and 4800.  A sub-block whose mean square
 * is at least SDRFM_LD_LOUD LSB^2 counts towards the relative figure |d| / e, any other towards the absolute one |d| / block_len, as in
 * tests/loudness_cases.py.  There a set is IN DOMAIN when both figures, measured over more rows than these, are at most an eighth of what
 * would hide a lost sample (1e-9 and 1e-3 LSB^2 per sample): the device's evaluation order then has a factor of eight to itself.  The
 * predicate asks for half of that, a sixteenth, because the figure behind a burst moves with the burst's samples — by 1.3 on the one set of
 * the tests' grid where it decides — and the probe tries one burst.  About 4e5 filter steps: some 8 ms per call. */
#define SDRFM_LD_LOUD 1e6
#define SDRFM_LD_ACCEPT_REL (1.25e-10 / 2.0)
#define SDRFM_LD_ACCEPT_ABS (1.25e-4 / 2.0)
#define SDRFM_LD_PROBE_CALL 4800u
#define SDRFM_LD_PROBE_LONG (2u * SDRFM_LD_TILE + 17u)
#define SDRFM_LD_PROBE_MAX (SDRFM_LD_PROBE_LONG > SDRFM_LD_PROBE_CALL ? SDRFM_LD_PROBE_LONG : SDRFM_LD_PROBE_CALL)   /* the longest call of the probe */

/* one call of the kernel on one channel: x[n] from the state (z[4], *e, *pos) -> the energies of the sub-blocks it completes, in out; returns
 * how many.  Every sum in the kernel's order: pass 1, the scan's combine, pass 2's two pieces, the pieces in lane order */
static inline uint32_t ld_emulate_channel(const double* c, const double* pw, const int16_t* x, uint32_t n, uint32_t B, double* z, double* e,
                                          uint64_t* pos, double* out) {
  double zz[2][SDRFM_LD_NT][4], piece[2][SDRFM_LD_NT];
  const double kappa = pw[16u * SDRFM_LD_STEPS], rkappa = pw[16u * SDRFM_LD_STEPS + 1u];
  uint32_t off = (uint32_t)(*pos % B), done = 0;
  for (uint32_t t = 0; t < ld_tiles(n); ++t) {
    const int16_t* xt = x + (size_t)t * SDRFM_LD_TILE;
    const uint32_t m = ld_tile_len(n, t), nact = ld_active_lanes(m);
    uint32_t cb, len, cur = 0;
    for (uint32_t j = 0; j < nact; ++j) {                        /* pass 1 */
      double* q = zz[0][j];
      ld_chunk(m, j, &cb, &len);
      for (int k = 0; k < 4; ++k) q[k] = j == 0 ? z[k] : 0.0;
      for (uint32_t i = 0; i < len; ++i) (void)ld_kw_step(c, q, (double)xt[cb + i]);
      q[3] = kappa * (q[2] + q[3]);
    }
    for (uint32_t s = 0; (1u << s) < nact; ++s) {                /* the scan */
      const uint32_t d = 1u << s;
      for (uint32_t j = 0; j < nact; ++j) {
        for (int k = 0; k < 4; ++k) zz[cur ^ 1u][j][k] = zz[cur][j][k];
        if (j >= d) ld_matvec_add(pw + 16u * s, zz[cur][j - d], zz[cur ^ 1u][j]);
      }
      cur ^= 1u;
    }
    double zn[4] = {0.0, 0.0, 0.0, 0.0};
    for (uint32_t j = 0; j < nact; ++j) {                        /* pass 2 */
      double q[4], e0 = 0.0, e1 = 0.0;
      ld_chunk(m, j, &cb, &len);
      for (int k = 0; k < 4; ++k) q[k] = j == 0 ? z[k] : zz[cur][j - 1u][k];
      if (j) q[3] = q[3] * rkappa - q[2];
      const uint32_t split = ld_split((off + cb) % B, B, len);
      for (uint32_t i = 0; i < len; ++i) {
        const double y = ld_kw_step(c, q, (double)xt[cb + i]);
        const double sq = y * y;
        if (i < split) e0 = e0 + sq;
        else e1 = e1 + sq;
      }
      piece[0][j] = e0;
      piece[1][j] = e1;
      if (j + 1u == nact)
        for (int k = 0; k < 4; ++k) zn[k] = q[k];
    }
    for (int k = 0; k < 4; ++k) z[k] = zn[k];
    const uint32_t nb = ld_tile_blocks(off, m, B);
    for (uint32_t k = 0; k <= nb; ++k) {                         /* the sub-blocks */
      int64_t start;
      uint32_t lo, hi;
      ld_block_span(off, m, B, k, &start, &lo, &hi);
      double acc = k == 0 ? *e : 0.0;
      if (hi > lo)
        for (uint32_t j = lo / SDRFM_LD_L; j <= (hi - 1u) / SDRFM_LD_L; ++j) acc = acc + piece[ld_piece(j, start)][j];
      if (k < nb) out[done++] = acc;
      else *e = acc;
    }
    off = ld_tile_next_off(off, m, B);
  }
  *pos += n;
  return done;
}

/* the same call by the definition, one sample after the other (sdrfm_pcm_loudness_s16's loop for one channel) */
static inline uint32_t ld_reference_channel(const double* c, const int16_t* x, uint32_t n, uint32_t B, double* z, double* e, uint64_t* pos,
                                            double* out) {
  uint32_t left = B - (uint32_t)(*pos % B), done = 0;
  for (uint32_t i = 0; i < n; ++i) {
    const double y = ld_kw_step(c, z, (double)x[i]);
    *e = *e + y * y;
    if (--left == 0) {
      out[done++] = *e;
      *e = 0.0;
      left = B;
    }
  }
  *pos += n;
  return done;
}

/* the two figures of a set over the probe's rows.  pw = ld_matrix_powers(c) */
enum { LD_P_END = 0, LD_P_ZERO, LD_P_DC, LD_P_NOISE };
typedef struct ld_probe_call { uint32_t what, n; } ld_probe_call;
#define SDRFM_LD_PROBE_ROWS 5

static inline void ld_probe(const double* c, const double* pw, double* rel, double* ab) {
  static const ld_probe_call rows[SDRFM_LD_PROBE_ROWS][4] = {
      {{LD_P_DC, SDRFM_LD_PROBE_CALL}, {LD_P_DC, SDRFM_LD_PROBE_CALL}, {LD_P_END, 0u}, {LD_P_END, 0u}},
      {{LD_P_DC, SDRFM_LD_PROBE_LONG}, {LD_P_END, 0u}, {LD_P_END, 0u}, {LD_P_END, 0u}},
      {{LD_P_DC, SDRFM_LD_PROBE_CALL}, {LD_P_ZERO, SDRFM_LD_PROBE_CALL}, {LD_P_ZERO, SDRFM_LD_PROBE_CALL}, {LD_P_ZERO, SDRFM_LD_PROBE_CALL}},
      {{LD_P_NOISE, SDRFM_LD_PROBE_CALL}, {LD_P_ZERO, SDRFM_LD_PROBE_CALL}, {LD_P_ZERO, SDRFM_LD_PROBE_CALL}, {LD_P_ZERO, SDRFM_LD_PROBE_CALL}},
      {{LD_P_NOISE, SDRFM_LD_TILE + 1u}, {LD_P_END, 0u}, {LD_P_END, 0u}, {LD_P_END, 0u}}};
  static const uint32_t block_lens[2] = {SDRFM_LD_BLOCK_MIN, 4800u};
  int16_t x[SDRFM_LD_PROBE_MAX];
  double got[SDRFM_LD_PROBE_MAX / SDRFM_LD_BLOCK_MIN + 1u], want[SDRFM_LD_PROBE_MAX / SDRFM_LD_BLOCK_MIN + 1u];
  *rel = *ab = 0.0;
  for (int b = 0; b < 2; ++b)
    for (int row = 0; row < SDRFM_LD_PROBE_ROWS; ++row) {
      const uint32_t B = block_lens[b];
      double zg[4] = {0.0, 0.0, 0.0, 0.0}, zw[4] = {0.0, 0.0, 0.0, 0.0}, eg = 0.0, ew = 0.0;
      uint64_t pos_g = 0, pos_w = 0, lcg = 0x9E3779B97F4A7C15ull + (uint64_t)row;
      for (int call = 0; call < 4 && rows[row][call].what != LD_P_END; ++call) {
        const uint32_t what = rows[row][call].what, n = rows[row][call].n;
        for (uint32_t i = 0; i < n; ++i) {
          if (what == LD_P_ZERO) x[i] = 0;
          else if (what == LD_P_DC) x[i] = 32767;
          else {
            lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
            x[i] = (int16_t)(uint16_t)(lcg >> 48);                           /* full range: the top 16 bits as a two's-complement int16 */
          }
        }
        const uint32_t k = ld_emulate_channel(c, pw, x, n, B, zg, &eg, &pos_g, got);
        (void)ld_reference_channel(c, x, n, B, zw, &ew, &pos_w, want);
        for (uint32_t i = 0; i < k; ++i) {
          const double d = got[i] > want[i] ? got[i] - want[i] : want[i] - got[i];
          if (!(d == d)) { *rel = *ab = 1.0; return; }                       /* NaN: a set whose sums overflow is in no domain */
          if (want[i] >= SDRFM_LD_LOUD * (double)B) { if (d / want[i] > *rel) *rel = d / want[i]; }
          else if (d / (double)B > *ab) *ab = d / (double)B;
        }
      }
    }
}

/* the predicate; the two figures go to rel and ab where those are not NULL */
static inline int ld_in_domain(const double* c, const double* pw, double* rel, double* ab) {
  double r, a;
  ld_probe(c, pw, &r, &a);
  if (rel) *rel = r;
  if (ab) *ab = a;
  return r <= SDRFM_LD_ACCEPT_REL && a <= SDRFM_LD_ACCEPT_ABS;
}

#if defined(__HIPCC__)

struct LoudnessParams {
  const int16_t* pcm;
  size_t pcm_stride;               /* int16 elements per stream, even; rows are 4-byte aligned */
  sdrfm_loudness_state* state;     /* [n_streams] */
  sdrfm_loudness_block* ring;      /* [n_streams][cap_blocks] */
  const double* pw;                /* [SDRFM_LD_TABLE]: ld_matrix_powers */
  sdrfm_loudness_coef coef;
  uint64_t blk0, keep_from;        /* pos / block_len before the call; the first sub-block index the call stores */
  uint32_t n, block_len, cap_blocks, off0;   /* off0 = pos % block_len before the call */
};

struct LoudnessShared {
  unsigned x[SDRFM_LD_TILE];                 /* the tile, L | R << 16 */
  double p[2][8][SDRFM_LD_NT];               /* the scan's two buffers, component-major; the free one then holds the lanes' four pieces */
  double pw[SDRFM_LD_TABLE];                 /* the table: read from here it lands in vector registers, where there is room */
  double c[10];                              /* the coefficients, for the same reason */
  double cz[8];                              /* the state carried into the next tile */
  double ce[2][2];                           /* the open sub-block's energy carried into tile t, [t & 1][channel] */
};

/* One workgroup of SDRFM_LD_NT lanes per stream. */
__device__ __forceinline__ void loudness_stream(LoudnessShared& sh, const LoudnessParams& p) {
  const uint32_t tid = threadIdx.x;
  const unsigned* row = reinterpret_cast<const unsigned*>(p.pcm + (size_t)blockIdx.x * p.pcm_stride);
  sdrfm_loudness_state* st = p.state + blockIdx.x;
  double* ring = reinterpret_cast<double*>(p.ring + (size_t)blockIdx.x * p.cap_blocks);
  const uint32_t B = p.block_len, n = p.n;
  const uint32_t ntiles = ld_tiles(n);
  uint32_t off = p.off0;
  uint64_t blk = p.blk0;
  if (tid < SDRFM_LD_TABLE) sh.pw[tid] = p.pw[tid];              /* these four are visible behind the first tile's barrier */
  if (tid < 10u) sh.c[tid] = p.coef.c[tid];
  if (tid < 8u) sh.cz[tid] = st->z[tid >> 2][tid & 3u];
  if (tid < 2u) sh.ce[0][tid] = st->e[tid];
  for (uint32_t t = 0; t < ntiles; ++t) {
    const uint64_t base = (uint64_t)t * SDRFM_LD_TILE;
    const uint32_t m = ld_tile_len(n, t);
    const uint32_t nact = ld_active_lanes(m);
    const bool last = t + 1u == ntiles;
    for (uint32_t i = tid; i < m; i += SDRFM_LD_NT) sh.x[i] = row[base + i];   /* coalesced dwords, nothing behind the tile's m pairs */
    __syncthreads();
    double c[10], cz[8], ce[2];                                  /* what the stream, or the tile before, carries in */
#pragma unroll
    for (int k = 0; k < 10; ++k) c[k] = sh.c[k];
#pragma unroll
    for (int k = 0; k < 8; ++k) cz[k] = sh.cz[k];
    ce[0] = sh.ce[t & 1u][0];
    ce[1] = sh.ce[t & 1u][1];
    uint32_t cb, len;
    ld_chunk(m, tid, &cb, &len);
    /* pass 1: the chunk from zero state; lane 0 from the carried state */
    double z[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) z[k] = tid == 0 ? cz[k] : 0.0;
#pragma unroll
    for (uint32_t i = 0; i < SDRFM_LD_L; ++i) {
      if (i < len) {
        const unsigned w = sh.x[cb + i];
        (void)ld_kw_step(c, z, (double)(int)(int16_t)(w & 0xFFFFu));
        (void)ld_kw_step(c, z + 4, (double)((int)w >> 16));
      }
    }
    /* into the scan's coordinates */
    {
      const double kappa = sh.pw[SDRFM_LD_STEPS * 16u];
      z[3] = kappa * (z[2] + z[3]);
      z[7] = kappa * (z[6] + z[7]);
    }
    /* the scan: after step i lane j holds the state its chunk and the 2^(i+1) - 1 before it leave */
    uint32_t cur = 0;
    for (uint32_t s = 0; (1u << s) < nact; ++s) {
      const uint32_t d = 1u << s;
#pragma unroll
      for (int k = 0; k < 8; ++k) sh.p[cur][k][tid] = z[k];
      __syncthreads();
      if (tid >= d && tid < nact) {
        double q[8], M[16];
#pragma unroll
        for (int k = 0; k < 8; ++k) q[k] = sh.p[cur][k][tid - d];
#pragma unroll
        for (int k = 0; k < 16; ++k) M[k] = sh.pw[16u * s + k];
        ld_matvec_add(M, q, z);
        ld_matvec_add(M, q + 4, z + 4);
      }
      cur ^= 1u;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) sh.p[cur][k][tid] = z[k];
    __syncthreads();
    /* pass 2: from the true incoming state, the state the lane before leaves, back in the filter's coordinates */
#pragma unroll
    for (int k = 0; k < 8; ++k) z[k] = sh.p[cur][k][tid - (tid ? 1u : 0u)];
    {
      const double rkappa = sh.pw[SDRFM_LD_STEPS * 16u + 1u];
      z[3] = z[3] * rkappa - z[2];
      z[7] = z[7] * rkappa - z[6];
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) z[k] = tid == 0 ? cz[k] : z[k];
    const uint32_t split = ld_split((off + cb) % B, B, len);
    double e[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
#pragma unroll
    for (uint32_t i = 0; i < SDRFM_LD_L; ++i) {
      if (i < len) {
        const unsigned w = sh.x[cb + i];
        const double yl = ld_kw_step(c, z, (double)(int)(int16_t)(w & 0xFFFFu));
        const double yr = ld_kw_step(c, z + 4, (double)((int)w >> 16));
        const double sl = yl * yl, sr = yr * yr;
        if (i < split) { e[0][0] = e[0][0] + sl; e[0][1] = e[0][1] + sr; }
        else { e[1][0] = e[1][0] + sl; e[1][1] = e[1][1] + sr; }
      }
    }
    double (*piece)[SDRFM_LD_NT] = sh.p[cur ^ 1u];               /* [2 * part + channel][lane]; no lane reads this buffer any more */
    piece[0][tid] = e[0][0]; piece[1][tid] = e[0][1]; piece[2][tid] = e[1][0]; piece[3][tid] = e[1][1];
    if (tid + 1u == nact) {                                      /* the last active lane's end state: the stream's, or the next tile's */
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        if (last) st->z[k >> 2][k & 3] = z[k];
        else sh.cz[k] = z[k];
      }
    }
    __syncthreads();
    /* one lane per sub-block and channel: the carried energy first (sub-block 0), then the lanes' pieces in lane order */
    const uint32_t nb = ld_tile_blocks(off, m, B);
    const uint32_t ch = tid & 1u;
    for (uint32_t k = tid >> 1; k <= nb; k += SDRFM_LD_NT / 2u) {
      int64_t start;
      uint32_t lo, hi;
      ld_block_span(off, m, B, k, &start, &lo, &hi);
      double acc = k == 0 ? ce[ch] : 0.0;
      if (hi > lo) {
        const uint32_t j1 = (hi - 1u) / SDRFM_LD_L;
        uint32_t j = lo / SDRFM_LD_L;
        for (; j + 8u <= j1 + 1u; j += 8u) {                       /* eight reads in flight, added in lane order all the same */
          double v[8];
#pragma unroll
          for (uint32_t u = 0; u < 8u; ++u) v[u] = piece[2u * ld_piece(j + u, start) + ch][j + u];
#pragma unroll
          for (uint32_t u = 0; u < 8u; ++u) acc = acc + v[u];
        }
        for (; j <= j1; ++j) acc = acc + piece[2u * ld_piece(j, start) + ch][j];
      }
      if (k < nb) {
        const uint64_t b = blk + k;
        if (b >= p.keep_from) ring[2u * (size_t)ld_ring_slot(b, p.cap_blocks) + ch] = acc;
      } else if (last) st->e[ch] = acc;
      else sh.ce[(t + 1u) & 1u][ch] = acc;
    }
    blk += nb;
    off = ld_tile_next_off(off, m, B);
  }
  if (tid == 0) st->pos = st->pos + n;
}

#endif /* __HIPCC__ */
#endif
