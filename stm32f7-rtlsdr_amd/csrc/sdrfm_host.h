/*
 * sdrfm_host.h — the host plumbing the handles beside the demodulators share: the HIP error macro, the quiet device check, a
 * handle's stream, the staging of a host-buffer call and the read-out of per-stream records.  Small free functions that each do one thing; every
 * extern "C" entry stays a plain function in its own file with its checks written out.  Internal, host code only, included by .hip files.
 */
#ifndef SDRFM_HOST_H
#define SDRFM_HOST_H

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/sdrfm.h"
#include "sdrfm_pcm_rows.h"

#define STRY(expr, code)                                                                                       \
  do {                                                                                                         \
    hipError_t e__ = (expr);                                                                                   \
    if (e__ != hipSuccess) {                                                                                   \
      fprintf(stderr, "[sdrfm] %s failed: %s (%s:%d)\n", #expr, hipGetErrorString(e__), __FILE__, __LINE__);  \
      return (code);                                                                                           \
    }                                                                                                          \
  } while (0)

// makes `device` current if it is a gfx950, without a word on stderr: SDRFM_OK or SDRFM_NO_DEVICE.  prop: the device's properties, where wanted
static inline int host_open_device(int device, hipDeviceProp_t* prop = nullptr) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return SDRFM_NO_DEVICE;
  hipDeviceProp_t mine;
  if (!prop) prop = &mine;
  if (hipGetDeviceProperties(prop, device) != hipSuccess || strncmp(prop->gcnArchName, "gfx950", 6) != 0) return SDRFM_NO_DEVICE;
  STRY(hipSetDevice(device), SDRFM_NO_DEVICE);
  return SDRFM_OK;
}

// ---- a handle's stream: its own, non-blocking, until the caller gives it another ----------------------------------------------------------
struct HostStream {
  int device;
  hipStream_t own, cur;
};

// on the current device (host_open_device); a failure counts as out of memory, as every create has answered it
static inline int host_stream_open(HostStream& s, int device) {
  s.device = device;
  if (hipStreamCreateWithFlags(&s.own, hipStreamNonBlocking) != hipSuccess) { s.own = nullptr; return SDRFM_ENOMEM; }
  s.cur = s.own;
  return SDRFM_OK;
}

static inline void host_stream_close(HostStream& s) {
  if (s.own) (void)hipStreamDestroy(s.own);
  s.own = s.cur = nullptr;
}

// the device current and everything enqueued on the stream done
static inline int host_stream_wait(HostStream& s) {
  STRY(hipSetDevice(s.device), SDRFM_FAIL);
  STRY(hipStreamSynchronize(s.cur), SDRFM_FAIL);
  return SDRFM_OK;
}

// waits for the stream in use, then switches: hip_stream, or NULL for the handle's own
static inline int host_stream_use(HostStream& s, void* hip_stream) {
  const int rc = host_stream_wait(s);
  if (rc != SDRFM_OK) return rc;
  s.cur = hip_stream ? static_cast<hipStream_t>(hip_stream) : s.own;
  return SDRFM_OK;
}

// ---- the staging of a host-buffer call: rows in on the device, rows out on the device, and where the handle asks for it a host copy of the
// rows out, from which every caller's row receives exactly its valid elements ------------------------------------------------------------------
struct RowStage {
  void* d_in;
  void* d_out;                     // d_in again where the shape has no rows out of its own
  void* h_out;
  uint32_t cap_in, cap_out;        // elements per row
};

// what a handle stages, fixed at create.  Sizes in bytes per element, so one function serves float rows, (L, R) pairs and raw bytes
struct RowShape {
  uint32_t round;                  // capacities are multiples of this many elements (a power of two: stage_cap)
  size_t in_elem, in_rows;
  size_t out_elem, out_rows;       // out_rows == 0: the call works in place or returns no rows; d_out is d_in and cap_out is cap_in
  bool bounce;                     // keep h_out
};

static inline void row_stage_free(RowStage& st) {
  if (st.d_out && st.d_out != st.d_in) (void)hipFree(st.d_out);
  if (st.d_in) (void)hipFree(st.d_in);
  free(st.h_out);
  st = RowStage{};
}

// room for n_in and n_out elements per row.  A side that is large enough stays; one that grows is freed first and allocated at stage_cap.  After a
// failure (SDRFM_ENOMEM) every pointer is null and both capacities are 0: the next call starts clean
static inline int row_stage_reserve(RowStage& st, const RowShape& sh, uint32_t n_in, uint32_t n_out) {
  const bool in_place = sh.out_rows == 0;
  bool ok = true;
  if (n_in > st.cap_in) {
    if (st.d_in) (void)hipFree(st.d_in);
    st.d_in = nullptr;
    st.cap_in = stage_cap(n_in, sh.round);
    ok = hipMalloc(&st.d_in, sh.in_elem * st.cap_in * sh.in_rows) == hipSuccess;
    if (in_place) {
      free(st.h_out);
      st.d_out = st.d_in; st.cap_out = st.cap_in;
      st.h_out = sh.bounce ? malloc(sh.in_elem * st.cap_in * sh.in_rows) : nullptr;
      ok = ok && (st.h_out || !sh.bounce);
    }
  }
  if (ok && !in_place && n_out > st.cap_out) {
    if (st.d_out) (void)hipFree(st.d_out);
    free(st.h_out);
    st.d_out = nullptr;
    st.cap_out = stage_cap(n_out, sh.round);
    st.h_out = sh.bounce ? malloc(sh.out_elem * st.cap_out * sh.out_rows) : nullptr;
    ok = (st.h_out || !sh.bounce) && hipMalloc(&st.d_out, sh.out_elem * st.cap_out * sh.out_rows) == hipSuccess;
  }
  if (ok) return SDRFM_OK;
  row_stage_free(st);
  return SDRFM_ENOMEM;
}

// host rows, src_pitch bytes apart, -> `rows` rows of the staging's input from row row0 on, `width` bytes each, enqueued on stream
static inline int rows_to_device(const RowStage& st, size_t elem, size_t row0, const void* src, size_t src_pitch, size_t width, size_t rows,
                                 hipStream_t stream) {
  STRY(hipMemcpy2DAsync(static_cast<char*>(st.d_in) + row0 * elem * st.cap_in, elem * st.cap_in, src, src_pitch, width, rows, hipMemcpyHostToDevice,
                        stream), SDRFM_FAIL);
  return SDRFM_OK;
}

// the staging's output rows -> host rows dst_pitch bytes apart, and the stream waited for: row r receives its first cnt[r] elements (n where cnt is
// NULL), through h_out where the staging keeps one — exactly those bytes, so a caller's last row may end with its data
static inline int rows_to_host(const RowStage& st, size_t elem, void* dst, size_t dst_pitch, uint32_t n, const uint32_t* cnt, size_t rows,
                               hipStream_t stream) {
  void* const to = st.h_out ? st.h_out : dst;
  if (n) STRY(hipMemcpy2DAsync(to, st.h_out ? elem * st.cap_out : dst_pitch, st.d_out, elem * st.cap_out, elem * n, rows, hipMemcpyDeviceToHost, stream),
              SDRFM_FAIL);
  STRY(hipStreamSynchronize(stream), SDRFM_FAIL);
  for (size_t r = 0; st.h_out && r < rows; ++r) {
    const uint32_t len = cnt ? cnt[r] : n;
    if (len) memcpy(static_cast<char*>(dst) + r * dst_pitch, static_cast<const char*>(st.h_out) + r * elem * st.cap_out, elem * len);
  }
  return SDRFM_OK;
}

// ---- the read-out of a handle's per-stream records, flags SDRFM_F_DEVICE_PTRS | SDRFM_AMETER_F_RESET (the entry has checked them): with device
// pointers the copy, and the reset if asked for, are enqueued on the handle's stream and nowhere else; else the call waits, copies, resets and
// waits.  A reset puts `identity` back (host memory the handle keeps), or zeroes where that is NULL ---------------------------------------------
static inline int records_read(HostStream& s, void* out, void* d_rec, size_t bytes, const void* identity, uint32_t flags) {
  STRY(hipSetDevice(s.device), SDRFM_FAIL);
  const bool host = !(flags & SDRFM_F_DEVICE_PTRS);
  if (host) {
    STRY(hipStreamSynchronize(s.cur), SDRFM_FAIL);
    STRY(hipMemcpy(out, d_rec, bytes, hipMemcpyDeviceToHost), SDRFM_FAIL);
  } else {
    STRY(hipMemcpyAsync(out, d_rec, bytes, hipMemcpyDeviceToDevice, s.cur), SDRFM_FAIL);
  }
  if (!(flags & SDRFM_AMETER_F_RESET)) return SDRFM_OK;
  if (identity) STRY(hipMemcpyAsync(d_rec, identity, bytes, hipMemcpyHostToDevice, s.cur), SDRFM_FAIL);
  else STRY(hipMemsetAsync(d_rec, 0, bytes, s.cur), SDRFM_FAIL);
  if (host) STRY(hipStreamSynchronize(s.cur), SDRFM_FAIL);
  return SDRFM_OK;
}

#endif
