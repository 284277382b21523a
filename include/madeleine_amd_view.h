/*
 * madeleine_amd_view.h -- the viewing side of libmadeleine_amd.so (gfx950 / MI355X): what turns the read-outs of madeleine_amd.h
 * into images.  A second header of the same library, the same conventions and the same strict grammar (madeleine_amd.h, top): extern
 * "C", plain pointers and sizes, device pointers unless the name ends in _host, caller-allocated buffers, asynchronous launches on
 * the caller's stream, 0 / positive hipError_t / negative MDL_E_* as the return value.  It declares entry points only; the MDL_E_*
 * codes and MDL_ABI_VERSION are those of madeleine_amd.h, and adding to THIS header does not change that revision: a binding checks
 * every name below against the loaded library by itself (a missing symbol is an error).
 *
 * V1 -- attention heatmaps: patch coordinates and per-patch values of a packed set of bags become RGBA images.  Replaces the host loop
 * every ABMIL user writes around the scores MADELEINE.forward(..., return_attention=True) returns (Model.py:205-216): average the
 * patch scores over overlapping patch footprints on a down-sampled canvas, blur, colour-map, blend over a thumbnail (the CLAM-style
 * heatmap).  The contract is EXACT INTEGER ARITHMETIC: a numpy int64 / uint64 restatement (tests/_heat_ref.py) equals the device
 * bit for bit.
 *
 * One call renders R bags x C channels.
 *   xy [T, 2] int32: (x, y) of every patch, level-0 pixels, top-left corner.  cu [R + 1] int64: bag b is rows cu[b] .. cu[b + 1] - 1.
 *   values [T, C] fp32, row stride ld >= C ELEMENTS: the extent is (T - 1) * ld + C elements and only the first C of a row are read.
 *   bag [R, MDL_HEAT_REC] int64, the per-bag record, given TWICE with the same contents: bag_host (host memory: validated, and the
 *     launch grids are sized from it) and bag (device: what the kernels read).  Fields: MDL_HEAT_PS patch side in level-0 pixels,
 *     MDL_HEAT_OX / MDL_HEAT_OY the level-0 origin of the canvas, MDL_HEAT_W / MDL_HEAT_H the canvas size in canvas pixels,
 *     MDL_HEAT_OFF the bag's first pixel in the packed planes.  P = the pixels of the packed planes; bag b owns pixels
 *     off .. off + W * H - 1, which must lie inside [0, P).
 *   ds >= 1: level-0 pixels per canvas pixel, call-wide.  taps_host [2 r + 1] int32 (host memory), r in [0, MDL_HEAT_MAX_R].
 *   lut [256, 4] uint8 (RGBA).  base [P, 3] uint8 or NULL: bag b's thumbnail is [H, W, 3] at byte 3 * off.  alpha in 0 .. 255.
 *   level uint16 [C * P], covered uint8 [C * P], rgba uint8 [C * P, 4]: bag b's block of each is [C, H, W] (rgba: [C, H, W, 4]) and
 *     starts at element C * off.  Nothing outside the blocks of the bags is written.
 *   ws: mdl_heat_ws_bytes(P, R, C) bytes, 16-byte aligned, contents need no initialisation.
 *
 * Steps.
 *   1 quantise.   NaN: the patch is left out of that channel.  v <= 0 (-0.0 and -inf included): q = 0.  v >= 1 (+inf included):
 *                 q = 65535.  Otherwise q = rint(fl32(v * 65535)), one fp32 product, round half to even.
 *   2 footprint.  Patch i of bag b covers the canvas pixels x in [floor((cx - ox) / ds), floor((cx - ox + ps - 1) / ds)] and y
 *                 likewise: FLOOR division, also of a negative numerator, in 64 bits.  Clipped to [0, W) x [0, H); a patch wholly
 *                 outside contributes nothing.
 *   3 accumulate. Per pixel and channel S = sum q and N = the number of contributing patches, as ONE 64-bit integer atomic add of
 *                 (1 << 40) + q into a packed word (N in bits 40 .. 63, S below): T < 2^24 keeps both fields exact.  Integer sums do
 *                 not depend on arrival order.
 *   4 blur.       taps are non-negative, symmetric, sum to MDL_HEAT_TAP_SUM = 4096 and have a centre > 0.  A row pass, then a column
 *                 pass, zeros outside the canvas, over S and over N separately in uint64: S1[y, x] = sum_k taps[k] * S[y, x + k - r],
 *                 S2[y, x] = sum_k taps[k] * S1[y + k - r, x], and N1, N2 alike.  S2 < 2^40 * 2^24: no overflow.  r = 0 multiplies
 *                 both by 4096^2: the identity of step 5.
 *   5 level.      Where N > 0 (the unblurred count): m = floor(S2 / N2), in 0 .. 65535 (N2 >= centre^2 * N > 0); level = m and
 *                 covered = 1.  Elsewhere the pixel is uncovered: level = 0, covered = 0.
 *   6 colour.     idx = (m * 255 + 32767) / 65535 and a = (lut[idx].a * alpha + 127) / 255, integer divisions.
 *                 Without base: RGBA = (lut[idx].rgb, a) where covered, (0, 0, 0, 0) elsewhere.
 *                 With base: rgb = (lut[idx].rgb * a + base.rgb * (255 - a) + 127) / 255 and alpha 255 where covered, (base.rgb, 255)
 *                 elsewhere.
 *
 * Kernels (csrc/heat_map.hip).  A canvas is cut into tiles of MDL_HEAT_TILE x MDL_HEAT_TILE pixels; hv_plan (one workgroup) turns
 * the records into the tile table, and a record that does not hold (below) is an EMPTY canvas on the device: nothing of it is read or
 * written.  hv_accumulate: a group of 1 .. 64 lanes per patch (a power of two, from the widest footprint of the call) walks the
 * footprint row-major, so that the lanes of one atomic instruction touch consecutive words of a canvas row, once per channel.
 * hv_blur_rows: a tile with a halo of r columns through LDS -> S1, N1.  hv_blur_cols: a tile with a halo of r rows through LDS, then
 * steps 5 and 6 and the three stores.  One memset of the packed words + four launches, whatever R, T and C; no workgroup waits on
 * another, no float atomics, no host read, no allocation.
 * Bit contract: a bag's images depend on its own rows, record and the call-wide ds / taps / lut / alpha alone -- not on R, on the
 * other bags, on where the bag lies in the call or on ld.
 *
 * Refusals, in this order, all before any launch and before any device pointer is touched.
 *   (1) MDL_E_ARG: cu / bag_host / bag / taps_host / lut / level / covered / rgba / ws NULL, xy / values NULL with T != 0 (with no row
 *       at all they may be: the canvases are still rendered, uncovered), T < 0, R < 0, C < 1, P < 0, ld < C, ds < 1, r < 0, alpha
 *       outside 0 .. 255.
 *   (2) MDL_E_UNSUPPORTED: r > MDL_HEAT_MAX_R; T >= 2^24; R or P beyond int32; C > 65535; C * P (the packed plane count) beyond int32.
 *   (3) MDL_E_ARG: a tap negative, the taps asymmetric, not summing to MDL_HEAT_TAP_SUM, or a centre of 0.
 *   (4) the records of bag_host in bag order, each: MDL_E_ARG for ps < 1, W < 1, H < 1 or off < 0; MDL_E_UNSUPPORTED for W or H >
 *       MDL_HEAT_MAX_SIDE, ps > 2^24, ox or oy beyond int32; MDL_E_ARG for off + W * H > P.  Then MDL_E_UNSUPPORTED for a tile count
 *       beyond the int32 launch geometry.
 *   (5) MDL_E_ALIGN: ws not 16-byte aligned, cu / bag / bag_host not 8-byte, xy / values / taps_host / rgba not 4-byte, level not
 *       2-byte aligned.
 * R == 0 or P == 0: MDL_OK, nothing launched.  mdl_heat_ws_bytes returns the byte count, or the codes of (1) and (2) for its sizes.
 * mdl_heat_render_marked: the same call, which also records MDL_HEAT_MARKS caller-created hipEvent_t (marks_host, a HOST array of event
 * handles, none NULL: else MDL_E_ARG before anything else) on the stream: before the memset, after the tile table, after the
 * accumulation, after the row pass and after the column pass.  For measurement; when R == 0 or P == 0 nothing is recorded.
 * With a cu that is not monotone or leaves [0, T], or a device record that differs from bag_host, nothing outside the given buffers
 * is read or written: such a bag or canvas is served as an empty one.
 */
#ifndef MADELEINE_AMD_VIEW_H
#define MADELEINE_AMD_VIEW_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MDL_HEAT_REC 6
#define MDL_HEAT_PS 0
#define MDL_HEAT_OX 1
#define MDL_HEAT_OY 2
#define MDL_HEAT_W 3
#define MDL_HEAT_H 4
#define MDL_HEAT_OFF 5
#define MDL_HEAT_MAX_R 32
#define MDL_HEAT_MAX_SIDE 32768
#define MDL_HEAT_TAP_SUM 4096
#define MDL_HEAT_TILE 32
#define MDL_HEAT_WS_PER_PLANE_PIXEL 24
#define MDL_HEAT_MARKS 5
int64_t mdl_heat_ws_bytes(int64_t P, int64_t R, int C);
int mdl_heat_render(const int32_t* xy, const int64_t* cu, const float* values, int64_t ld, int64_t T, int64_t R, int C,
                    const int64_t* bag_host, const int64_t* bag, int64_t P, int ds, const int32_t* taps_host, int r, const uint8_t* lut,
                    const uint8_t* base, int alpha, uint16_t* level, uint8_t* covered, uint8_t* rgba, void* ws, void* stream);
int mdl_heat_render_marked(const int32_t* xy, const int64_t* cu, const float* values, int64_t ld, int64_t T, int64_t R, int C,
                           const int64_t* bag_host, const int64_t* bag, int64_t P, int ds, const int32_t* taps_host, int r,
                           const uint8_t* lut, const uint8_t* base, int alpha, uint16_t* level, uint8_t* covered, uint8_t* rgba, void* ws,
                           void* const* marks_host, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MADELEINE_AMD_VIEW_H */
