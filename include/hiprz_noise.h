/* hiprz_noise.h — the noise level of a frame: a per-tile error map in display units and its summary (libhiprz_noise.so).
 *
 * No counterpart in the reference, whose only answer to a noisy frame is more passes.  The library is a pure function of device images: it
 * knows nothing of hiprz_ctx.  A host feeds it hiprz_accum_device and hiprz_variance_device (include/hiprz.h) on hiprz_stream; a caller that
 * never asks for the noise level runs no code of this library.
 *
 * THE NOISE LEVEL, in fp32, deterministic (no atomics: the same bits on every run), every operation rounded separately.
 * Input: two row-major W*H float4 images on one device: the accumulator (R_r, R_g, R_b, A) as hiprz_read_accum defines it and the variance
 * estimate (V_r, V_g, V_b, K) as hiprz_read_variance defines it.
 *
 * Tiles are the renderer's 32x8 blocks of the image grid: tiles_x = ceil(W / 32), tiles_y = ceil(H / 8), tile t = ty * tiles_x + tx holds the
 * pixels x in 32 tx .. 32 tx + 31, y in 8 ty .. 8 ty + 7, pixel (x, y) on lane l = (y % 8) * 32 + (x % 32).
 *
 * Per pixel:
 *   k    = ((aperture * aperture * pi) * exposure_time) * 1e5          the k of the tone curve t(c) = kc / (kc + 1)  (pi rounded to fp32)
 *   a    = A == 0 ? 1 : A;   r_ch = R_ch / a                           (the tone map's own rule)
 *   d_ch = k * r_ch + 1;     s_ch = sqrt(V_ch) * (k / (d_ch * d_ch))   the standard deviation through the tone curve's slope t'(r) = k / (kr + 1)^2
 *   e    = (0.2126 s_r + 0.7152 s_g) + 0.0722 s_b                      lum of the channels' standard deviations: they are added, as the
 *                                                                      variance-guided filter's v_0 adds them (the upper bound for correlated channels)
 *   estimated = the pixel is in the frame && K >= min_batches && e is finite
 * e is the standard error of the pixel's displayed luminance, in display units (1 = the whole range, 1/255 = one step of RGBA8).
 * It is a linearisation: exact to a percent where light arrives along every path (next-event estimation), a LOWER BOUND where a pixel's
 * radiance is a few rare, very bright paths into a small emitter and its spread is wider than the knee of the tone curve — there it can
 * even rise with the passes at first (DESIGN.md "Noise level" has the measured ratios).
 *
 * Tile record, a float4: (sum of e^2, max of e, n_estimated, n_above), all four over the tile's estimated pixels; n_above counts those with
 * e > threshold.  A lane without an estimate (outside the frame included) contributes 0 to the sum, the max and the counts.
 *
 * The sum has a fixed order, so its bits depend neither on the run nor on the implementation:
 *   1. within each wave (wave w holds lanes 64 w .. 64 w + 63), for s = 32, 16, 8, 4, 2, 1:  v[l] += v[l + s] for l < s   (__shfl_down)
 *   2. then (w0 + w1) + (w2 + w3).
 *
 * The kernel (rz_noise_tiles_kernel): one workgroup of 256 threads per tile, two float4 loads per thread (32 consecutive lanes read 512
 * contiguous bytes of a row of each image), LDS for the four wave results only.
 *
 * THE SUMMARY, on the host in float64 over the tiles in index order:
 *   estimated = sum of n_estimated, above = sum of n_above, pixels = W * H
 *   rms = sqrt(sum of the tiles' sums / estimated), 0 when nothing is estimated
 *   max = the largest per-tile max
 *   tile_rms_max = the largest sqrt(sum / n_estimated) over the tiles with an estimate, worst_tile = its index (the first one on ties);
 *   both 0 when no tile has one.
 * A stopping rule reads tile_rms_max, not rms: noise concentrated in one region of the image is not averaged away by a clean background. */
#ifndef HIPRZ_NOISE_H
#define HIPRZ_NOISE_H

#include <stdint.h>

#include "hiprz.h" /* the return codes: HIPRZ_OK, HIPRZ_ERR_INVALID, HIPRZ_ERR_DEVICE */

#ifdef __cplusplus
extern "C" {
#endif

#define HIPRZ_NOISE_TILE_W 32u
#define HIPRZ_NOISE_TILE_H 8u

/* a device buffer of tile records and its pinned twin on the host, grown on demand; one call at a time per meter.  hiprz_noise_tiles and
 * hiprz_noise_measure make the meter's device the calling thread's current HIP device, as the calls of include/hiprz.h do with theirs. */
typedef struct hiprz_noise_meter hiprz_noise_meter;
int hiprz_noise_create(hiprz_noise_meter** out, int device_id);   /* HIPRZ_ERR_DEVICE without a usable HIP device of that id */
int hiprz_noise_destroy(hiprz_noise_meter* meter);
const char* hiprz_noise_last_error(const hiprz_noise_meter* meter);   /* NULL: the last error of a call without a meter, on this thread */

typedef struct hiprz_noise_params {
    float aperture, exposure_time;   /* the camera's: k of the tone curve */
    float threshold;                 /* display units; estimated pixels with e > threshold are counted in n_above */
    uint32_t min_batches;            /* >= 2: a pixel has an estimate when K >= min_batches */
} hiprz_noise_params;

/* Enqueue only, on `stream` (a hipStream_t, NULL = the device's default stream): tiles_out_device receives tiles_x * tiles_y float4 records.
 * HIPRZ_ERR_INVALID, before anything is launched, on a null meter, image, output or params, on images that overlap the output, on a zero
 * width or height, on min_batches < 2 and on a threshold, aperture or exposure_time that is negative or not finite. */
int hiprz_noise_tiles(hiprz_noise_meter* meter, const void* accum_image_device, const void* variance_image_device, uint32_t width,
                      uint32_t height, const hiprz_noise_params* params, void* tiles_out_device, void* stream);

typedef struct hiprz_noise_summary {
    double rms, tile_rms_max;
    float max;
    uint32_t worst_tile;
    uint64_t estimated, above, pixels;
    uint32_t tiles_x, tiles_y;
} hiprz_noise_summary;

/* The same into the meter's own buffer, copied to its pinned memory on `stream`; the stream is waited for and the records are summarised
 * on the host.  tiles_out_host: NULL, or room for tiles_x * tiles_y * 4 floats. */
int hiprz_noise_measure(hiprz_noise_meter* meter, const void* accum_image_device, const void* variance_image_device, uint32_t width,
                        uint32_t height, const hiprz_noise_params* params, void* stream, hiprz_noise_summary* out, float* tiles_out_host);

/* Pure host, no device: THE SUMMARY of tile records.  HIPRZ_ERR_INVALID on a null pointer, a zero size, or a tile grid that is not the
 * frame's (tiles_x != ceil(width / 32) or tiles_y != ceil(height / 8)). */
int hiprz_noise_summarise(const float* tiles, uint32_t tiles_x, uint32_t tiles_y, uint32_t width, uint32_t height, hiprz_noise_summary* out);

/* sizeof(hiprz_noise_params), sizeof(hiprz_noise_summary) and the offsets of hiprz_noise_summary::estimated and ::tiles_x as this library
 * was compiled */
void hiprz_noise_layout(uint32_t out[4]);

#ifdef __cplusplus
}
#endif
#endif
