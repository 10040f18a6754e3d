/*
 * sdrfm_sink_stereo.h — what the one-call forms sdrfm_stereo_process_batch_pcm and sdrfm_bcast_process_batch_pcm (sdrfm_stereo.hip,
 * sdrfm_bcast.hip) need of the device stereo PCM sink (sdrfm_sink_stereo.hip): its checks, its staging rows and its default kernel on a
 * stream of the caller's.  No part of the C-ABI.
 */
#ifndef SDRFM_SINK_STEREO_H
#define SDRFM_SINK_STEREO_H

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

struct sdrfm_pcm_stereo_sink;

// the sink's share of a one-call form's refusals, nothing touched: SDRFM_EINVAL for a sink of another device or stream count, then the
// PCM checks of sdrfm_pcm_stereo_sink_process_batch against the call's n outputs (none when n is 0)
int sdrfm_stereo_sink_check(const sdrfm_pcm_stereo_sink* k, int device, uint32_t n_streams, uint32_t n, const int16_t* pcm, size_t pcm_stride,
                            bool device_ptrs);
// host-buffer calls: staging rows for n outputs per stream (the device must be current); *d_pcm and its row stride in int16 elements
int sdrfm_stereo_sink_reserve(sdrfm_pcm_stereo_sink* k, uint32_t n, int16_t** d_pcm, size_t* d_pcm_stride);
// the default form over device rows, enqueued on `stream`; n == 0 launches nothing
int sdrfm_stereo_sink_launch_on(sdrfm_pcm_stereo_sink* k, const float* left, const float* right, size_t audio_stride, uint32_t n, int16_t* pcm,
                                size_t pcm_stride, hipStream_t stream);
// the staged PCM of n outputs per stream back to the caller's rows, enqueued on `stream`
int sdrfm_stereo_sink_copy_back(const sdrfm_pcm_stereo_sink* k, int16_t* pcm, size_t pcm_stride, uint32_t n, hipStream_t stream);

#endif
