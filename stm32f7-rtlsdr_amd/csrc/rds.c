/*
 * rds.c — the 1187.5 bit/s part of RDS reception (include/sdrfm.h): the complex baseband of sdrfm_rds_process_batch
 * in, groups out.  Plain C99, host only: a few thousand operations per second and stream, serial by nature.
 *
 * Per sample of w (every stage keeps its state in the object, so a cut into pushes changes nothing):
 *   axis     S = leaky mean of w^2; the data axis is arg(S) / 2, kept continuous (of the two unit vectors the one nearer the last
 *            one: the sign of a BPSK axis is free, but a flip would cost a differential bit).  x = Re(w conj(u)).
 *   symbol   y[n] = sum of x over the older half bit - sum over the newer half bit: the matched filter of a biphase symbol with
 *            rectangular halves.  |y| is full at the symbol instants whatever the data; half a bit off it is full or nothing.
 *   clock    a phase accumulator of 1 / (samples per bit) per sample; a bit is decided where it wraps.
 *            acquisition: the energy of y, binned by the clock's phase over the last bits (leaky); after 32 bits with signal the
 *                         clock jumps so that it wraps at the fullest bin.
 *            tracking:    early / late: |y| one step before and after the decision instant steer the phase by a first-order loop
 *                         (gain 0.02 bit per unit error: a +-100 ppm crystal, 1e-4 bit per bit, costs 0.005 bit of lag); should the
 *                         instant half a bit off carry more energy for 24 bits on end, the clock jumps half a bit.
 *   bits     e = sign(y) at the instant, b = e xor e_prev (the differential coding), shifted into a 26-bit register.
 *   blocks   out of sync, every bit: syndrome of the register; a hit (an offset word) counts only if the window 26 bits earlier hit
 *            the offset word that precedes it in A B C|C' D A.  A lone hit is chance: 5 of 1024 windows.  A false acquisition needs a
 *            hit and, 26 bits on, the one successor word (two for B -> C | C'): 5/1024 x 1.2/1024 = 5.7e-6 per bit of noise, 1.4 % per
 *            2 s.  In sync, every 26 bits: the block is ok if its syndrome is the expected offset word (C or C' in place 3).
 *            LOSS consecutive failed blocks drop the synchronisation; after 2, an in-sequence pair at another alignment moves it.
 */
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/sdrfm.h"

#define RDS_POLY 0x5B9u
#define RDS_BITRATE 1187.5
#define RDS_MAX_SPB 64
#define RDS_ACQ_BITS 32
#define RDS_LOSS 10
#define RDS_HALF_RUN 24

static const uint16_t OFFSET_WORD[5] = {0x0FC, 0x198, 0x168, 0x350, 0x1B4};   /* A B C C' D */
static const int OFFSET_PLACE[5] = {0, 1, 2, 2, 3};

uint16_t sdrfm_rds_syndrome(uint32_t block26) {
  uint32_t r = block26 & 0x3FFFFFFu;
  for (int i = 25; i >= 10; --i)
    if (r & (1u << i)) r ^= RDS_POLY << (i - 10);
  return (uint16_t)(r & 0x3FFu);
}

uint16_t sdrfm_rds_checkword(uint16_t info, int offset) {
  if (offset < 0 || offset > 4) return 0xFFFF;
  return (uint16_t)(sdrfm_rds_syndrome((uint32_t)info << 10) ^ OFFSET_WORD[offset]);
}

static int offset_of(uint16_t syn) {
  for (int o = 0; o < 5; ++o)
    if (syn == OFFSET_WORD[o]) return o;
  return -1;
}

struct sdrfm_rds_sync {
  double spb;                      /* samples per bit */
  int half, el, ring;              /* half a bit and the early / late step in samples; length of the rings */
  /* axis */
  double sr, si, ur, ui, alpha;
  /* symbol filter */
  double xr[2 * RDS_MAX_SPB + 2];  /* last `ring` x's */
  double yr[2 * RDS_MAX_SPB + 2];  /* last `ring` y's */
  uint32_t pos;
  double sum_old, sum_new;
  /* clock */
  double ph;
  int locked;
  uint32_t nb;
  double hist[RDS_MAX_SPB + 1];
  uint32_t acq_bits;
  double e_on, e_mid;
  uint32_t half_run;
  /* bits */
  int e_prev;
  uint64_t reg;                    /* the last 52 bits: the window and the one before it */
  uint64_t nbits;
  int8_t hits[26];
  /* blocks */
  int in_sync, place;              /* place: which block of the group the next 26 bits are */
  uint32_t fill, fails;
  sdrfm_rds_group grp;
  sdrfm_rds_sync_info st;
};

int sdrfm_rds_sync_reset(sdrfm_rds_sync_t* s) {
  if (!s) return SDRFM_EINVAL;
  const double spb = s->spb;
  memset(s, 0, sizeof *s);
  s->spb = spb;
  s->half = (int)floor(spb / 2.0 + 0.5);
  if (s->half < 1) s->half = 1;
  s->el = (int)floor(spb / 8.0 + 0.5);
  if (s->el < 1) s->el = 1;
  s->ring = 2 * s->half + 2 * s->el + 2;
  s->alpha = 1.0 / (32.0 * spb);
  s->ur = 1.0;
  s->nb = (uint32_t)ceil(spb);
  if (s->nb > RDS_MAX_SPB) s->nb = RDS_MAX_SPB;
  memset(s->hits, -1, sizeof s->hits);
  return SDRFM_OK;
}

int sdrfm_rds_sync_create(double sample_rate_hz, sdrfm_rds_sync_t** out) {
  if (!out) return SDRFM_EINVAL;
  *out = NULL;
  if (!(sample_rate_hz >= 4.0 * RDS_BITRATE) || !(sample_rate_hz <= RDS_MAX_SPB * RDS_BITRATE)) return SDRFM_EINVAL;
  sdrfm_rds_sync_t* s = (sdrfm_rds_sync_t*)calloc(1, sizeof *s);
  if (!s) return SDRFM_ENOMEM;
  s->spb = sample_rate_hz / RDS_BITRATE;
  (void)sdrfm_rds_sync_reset(s);
  *out = s;
  return SDRFM_OK;
}

void sdrfm_rds_sync_destroy(sdrfm_rds_sync_t* s) { free(s); }

int sdrfm_rds_sync_stats(const sdrfm_rds_sync_t* s, sdrfm_rds_sync_info* out) {
  if (!s || !out) return SDRFM_EINVAL;
  *out = s->st;
  out->in_sync = (uint32_t)s->in_sync;
  return SDRFM_OK;
}

typedef struct { sdrfm_rds_group* out; uint32_t cap, n; } sink_t;

static void emit(sdrfm_rds_sync_t* s, sink_t* k) {
  if (s->grp.ok_mask) {
    if (k->n < k->cap) k->out[k->n++] = s->grp;
    s->st.groups++;
  }
  memset(&s->grp, 0, sizeof s->grp);
}

static void put_block(sdrfm_rds_sync_t* s, int place, int off, uint16_t info, int ok) {
  s->grp.block[place] = info;
  if (ok) {
    s->grp.ok_mask |= (uint8_t)(1u << place);
    if (place == 2) s->grp.version_b = (uint8_t)(off == 3);
  }
}

/* o follows prev in the sequence A B C|C' D A */
static int follows(int prev, int o) { return OFFSET_PLACE[o] == ((OFFSET_PLACE[prev] + 1) & 3); }

static void on_bit(sdrfm_rds_sync_t* s, int bit, sink_t* k) {
  s->reg = ((s->reg << 1) | (uint64_t)bit) & 0xFFFFFFFFFFFFFull;
  const uint32_t slot = (uint32_t)(s->nbits % 26);
  s->nbits++;
  s->st.bits++;
  const uint16_t syn = sdrfm_rds_syndrome((uint32_t)(s->reg & 0x3FFFFFFu));
  const int o = s->nbits >= 26 ? offset_of(syn) : -1;
  const int before = s->hits[slot];                    /* the window that ended 26 bits ago */
  s->hits[slot] = (int8_t)o;
  const int pair = o >= 0 && before >= 0 && s->nbits >= 52 && follows(before, o);
  const uint16_t info = (uint16_t)((s->reg >> 10) & 0xFFFFu);

  if (s->in_sync) {
    if (++s->fill == 26) {
      s->fill = 0;
      const int ok = o >= 0 && OFFSET_PLACE[o] == s->place;
      put_block(s, s->place, o, info, ok);
      if (ok) { s->st.blocks_ok++; s->fails = 0; } else { s->st.blocks_failed++; s->fails++; }
      if (s->place == 3) emit(s, k);
      s->place = (s->place + 1) & 3;
      if (s->fails >= RDS_LOSS) { emit(s, k); s->in_sync = 0; }
      return;
    }
    if (!(pair && s->fails >= 2)) return;
    emit(s, k);                                        /* an in-sequence pair at another alignment while this one fails: move */
  }
  if (pair) {
    /* both blocks of the pair are reported: the earlier one's 26 bits are still in the register */
    s->in_sync = 1;
    s->fails = 0;
    s->fill = 0;
    memset(&s->grp, 0, sizeof s->grp);
    put_block(s, OFFSET_PLACE[before], before, (uint16_t)((s->reg >> 36) & 0xFFFFu), 1);
    if (OFFSET_PLACE[before] == 3) emit(s, k);
    put_block(s, OFFSET_PLACE[o], o, info, 1);
    s->st.blocks_ok += 2;
    if (OFFSET_PLACE[o] == 3) emit(s, k);
    s->place = (OFFSET_PLACE[o] + 1) & 3;
  }
}

static void on_sample(sdrfm_rds_sync_t* s, double wr, double wi, sink_t* k) {
  /* ---- axis */
  s->sr += s->alpha * ((wr * wr - wi * wi) - s->sr);
  s->si += s->alpha * (2.0 * wr * wi - s->si);
  const double r = hypot(s->sr, s->si);
  if (r > 0.0) {
    double c = sqrt(0.5 * (r + s->sr) / r), d = sqrt(0.5 * (r - s->sr) / r);
    if (s->si < 0.0) d = -d;
    if (c * s->ur + d * s->ui < 0.0) { c = -c; d = -d; }
    s->ur = c; s->ui = d;
  }
  const double x = wr * s->ur + wi * s->ui;
  /* ---- symbol filter: y = (x[n-2h+1 .. n-h]) - (x[n-h+1 .. n]) */
  const int R = s->ring, h = s->half;
  const uint32_t p = s->pos % (uint32_t)R;
  const double x_h = s->xr[(s->pos + (uint32_t)R - (uint32_t)h) % (uint32_t)R];          /* x[n-h] */
  const double x_2h = s->xr[(s->pos + (uint32_t)R - 2u * (uint32_t)h) % (uint32_t)R];    /* x[n-2h] */
  s->xr[p] = x;
  s->sum_new += x - x_h;
  s->sum_old += x_h - x_2h;
  if ((s->pos & 1023u) == 1023u) {                    /* running sums: rebuilt from the ring now and then, at fixed sample indexes */
    double a = 0.0, b = 0.0;
    for (int i = 0; i < h; ++i) {
      b += s->xr[(s->pos + (uint32_t)R - (uint32_t)i) % (uint32_t)R];
      a += s->xr[(s->pos + (uint32_t)R - (uint32_t)h - (uint32_t)i) % (uint32_t)R];
    }
    s->sum_new = b; s->sum_old = a;
  }
  const double y = s->sum_old - s->sum_new;
  s->yr[p] = y;
#define Y_AGO(k_) (s->yr[(s->pos + (uint32_t)R - (uint32_t)(k_)) % (uint32_t)R])
  /* ---- clock */
  s->ph += 1.0 / s->spb;
  int strobe = 0;
  if (s->ph >= 1.0) { s->ph -= 1.0; strobe = 1; }
  if (!s->locked) {
    uint32_t bin = (uint32_t)(s->ph * s->nb);
    if (bin >= s->nb) bin = s->nb - 1;
    s->hist[bin] += y * y;
    if (strobe) {
      double tot = 0.0;
      uint32_t best = 0;
      for (uint32_t i = 0; i < s->nb; ++i) {
        tot += s->hist[i];
        if (s->hist[i] > s->hist[best]) best = i;
      }
      if (tot > 0.0) s->acq_bits++;
      if (s->acq_bits >= RDS_ACQ_BITS) {
        /* the fullest bin's samples become the on-time ones: the clock wraps `el` samples after them */
        double shift = (1.0 - s->el / s->spb) - (best + 0.5) / s->nb;
        s->ph += shift;
        s->ph -= floor(s->ph);
        s->locked = 1;
        s->e_on = s->e_mid = 0.0;
        s->half_run = 0;
        strobe = 0;
      } else {
        for (uint32_t i = 0; i < s->nb; ++i) s->hist[i] *= 1.0 - 1.0 / RDS_ACQ_BITS;
      }
    }
  }
  if (strobe) {
    const double on = Y_AGO(s->el), early = Y_AGO(2 * s->el), late = Y_AGO(0), mid = Y_AGO(s->el + s->half);
    if (s->locked) {
      const double ae = fabs(early), al = fabs(late), den = ae + al;
      if (den > 0.0) s->ph -= 0.02 * (al - ae) / den;   /* late fuller: the instant lies later: hold the clock back */
      s->e_on += (on * on - s->e_on) / 16.0;
      s->e_mid += (mid * mid - s->e_mid) / 16.0;
      if (s->e_mid > s->e_on) {
        if (++s->half_run >= RDS_HALF_RUN) { s->ph += 0.5; if (s->ph >= 1.0) s->ph -= 1.0; s->half_run = 0; s->e_on = s->e_mid = 0.0; }
      } else {
        s->half_run = 0;
      }
    }
    const int e = on > 0.0;
    on_bit(s, e ^ s->e_prev, k);
    s->e_prev = e;
  }
#undef Y_AGO
  s->pos++;
}

int sdrfm_rds_sync_push(sdrfm_rds_sync_t* s, const float* bb, uint32_t n, sdrfm_rds_group* out, uint32_t cap, uint32_t* n_out) {
  if (!s || !n_out || (n && !bb) || (cap && !out)) return SDRFM_EINVAL;
  sink_t k = {out, cap, 0};
  for (uint32_t i = 0; i < n; ++i) {
    const double wr = bb[2 * i], wi = bb[2 * i + 1];
    if (!isfinite(wr) || !isfinite(wi)) { on_sample(s, 0.0, 0.0, &k); continue; }
    on_sample(s, wr, wi, &k);
  }
  *n_out = k.n;
  return SDRFM_OK;
}
