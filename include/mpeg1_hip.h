/* include/mpeg1_hip.h — C-ABI of the MI355X (gfx950) MPEG-1 I-frame hot path.
 *
 * This is the boundary a host program (C, JNI, cgo, ctypes ...) binds.  Plain pointers and sizes
 * only; no C++ or torch types.  Implemented by libencoder.so (ec504_imageencoder_amd/csrc/).
 *
 * What each entry point replaces in the reference (eburhansjah/ec504_ImageEncoder, paths under
 * /root/reference):
 *
 *   m1v_encode_device / m1v_encode_host
 *       the per-frame body of mpeg_encode_procedure, include/encoder.h:196-458:
 *       packet/sequence/GOP/picture headers (source/mpeg1_enc.c:47-129), convert_rgb_to_ycbcr
 *       (source/image_processing.c:68), the slice -> macroblock -> block loops (encoder.h:238-444:
 *       extract_8x8_block :138, fast_DCT :192, quantization :349, zigzag_scanning :373,
 *       run_length_encode :703, encode_block_header_i source/mpeg1_blk.c:67, VLC_encode
 *       image_processing.c:400, encode_blk_coeff source/vlc.c:315, bit_vector.c appends),
 *       the strip zero-padding (encoder.h:442), the 16-bit length back-patch (encoder.h:448-453)
 *       and the 4 trailing bytes (encoder.h:456-458).
 *   m1v_encode_planes_host     one frame-loop iteration per frame, complete: the frame record AND the planes that
 *                              write_to_bitstream (image_processing.c:753, called at encoder.h:461-465) stores
 *   m1v_encode_quality_device / m1v_frame_sizes_device / m1v_encode_budget_device
 *                              no reference counterpart (one quality per run there): per-frame quality, size probe, budget
 *   m1v_frame_size_table_device / m1v_encode_batch_budget_device / m1v_encode_cbr_device
 *                              no reference counterpart: sizes at up to 8 qualities, a byte budget for a whole batch, a
 *                              constant bitrate through a leaky bucket
 *   m1v_frame_rd_table_device / m1v_encode_rd_device
 *                              no reference counterpart: the distortion beside the size at up to 8 qualities, and encodes that
 *                              pick per frame by both
 *   m1v_set_pipelined / m1v_flush   no reference counterpart: overlap of one batch's gather with the next encode
 *   m1v_warm_up, m1v_alloc_host/_free_host   no reference counterpart: runtime start-up off the critical path, pinned buffers
 *   m1v_coefficients_device    fast_DCT + quantization + zigzag_scanning only (BASELINE config 2)
 *   m1v_convert_device/_host   convert_rgb_to_ycbcr, image_processing.c:68-110 (feeds the .bit files,
 *                              write_to_bitstream image_processing.c:753)
 *   m1v_subsample_device       subsampling_420, image_processing.c:114-133 (dead in the reference's
 *                              data flow; provided for completeness)
 *   m1v_file_prolog            mpeg1_file_header + mpeg1_sys_header, mpeg1_enc.c:7-44 / encoder.h:86-89
 *   m1v_synth_device           no reference counterpart: device-side synthetic frames for benchmarks
 *
 * The coarse, drop-in entry point mpeg_encode_procedure() is declared in include/encoder.h.
 *
 * Threads: an m1v_encoder is used by one thread at a time (different encoders, also on the same GPU, may be
 * used concurrently); m1v_last_error() is per thread.
 *
 * All *_device entry points are asynchronous on `stream` (a hipStream_t passed as void*, NULL =
 * the default stream) and take DEVICE pointers.  Return value: M1V_OK or a negative M1V_E_*.
 */
#ifndef MPEG1_HIP_H
#define MPEG1_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Region covered by the macroblock loops:
 *   STRICT  x in [0,96), y in [0,144): the literals at encoder.h:238 / :248 (byte-identical to the
 *           unmodified reference)
 *   FULL    x in [0, W & ~15), y in [0, H & ~15): the reference with those two literals restored */
enum { M1V_MODE_STRICT = 0, M1V_MODE_FULL = 1 };

enum {
    M1V_OK = 0,
    M1V_E_ARG = -1,         /* bad argument / geometry the reference would read out of bounds with  */
    M1V_E_UNENCODABLE = -2, /* an emitted AC level has |level| >= 256 (reference: vlc.c:349 -> NULL
                               -> segfault); output of the batch is undefined                       */
    M1V_E_NOSPACE = -3,     /* output buffer too small                                             */
    M1V_E_HIP = -4,         /* HIP runtime error, see m1v_last_error()                             */
    M1V_E_NODEVICE = -5,    /* no usable gfx950 device                                             */
    M1V_E_SCRATCH = -6      /* the batch needs more scratch than reserved: m1v_reserve_scratch(enc, 1)
                               and encode again (the host-buffer entry points do so themselves)       */
};

/* bits of the device status word (m1v_encode_device's d_status) */
enum { M1V_STATUS_UNENCODABLE = 1u, M1V_STATUS_NOSPACE = 2u, M1V_STATUS_SCRATCH = 4u };
/* M1V_STATUS_QUALITY: a per-frame quality outside 1 .. the encoder's quality factor (output of the batch undefined);
 * M1V_STATUS_OVER_BUDGET (output valid): m1v_encode_budget_device found no candidate that fits some frame's budget,
 * m1v_encode_batch_budget_device found that even every frame at the smallest candidate exceeds the batch's budget, or
 * m1v_encode_cbr_device found no candidate that fits the buffer level of some frame */
enum { M1V_STATUS_QUALITY = 8u, M1V_STATUS_OVER_BUDGET = 16u };

typedef struct m1v_encoder m1v_encoder;

int m1v_device_count(void);
const char *m1v_last_error(void); /* thread-local, never NULL */

/* One encoder = one device, one picture geometry, one quality factor (the finest a frame of it can have: see
 * m1v_encode_quality_device).  max_frames bounds the batch
 * a single m1v_encode_* call may carry (scratch is sized for it).
 *
 * The long-batch rule.  Any positive max_frames is accepted, but one call carries at most m1v_batch_limit(enc) frames: the
 * smaller of max_frames and of the extents the device reports for a grid's y and z axes (hipDeviceAttributeMaxGridDimY / Z; the
 * assembly kernel takes the batch's frames as its grid's y, the run-shaped coefficient kernel as its grid's z).  Every call that
 * takes n_frames and is bound by max_frames, and m1v_coefficients_device where the run-shaped kernel serves it (4 channels, or a
 * path or input mode forced by a m1v_debug_set_* hook; its tile form has a one-dimensional grid and takes any n_frames), refuses
 * a longer batch with M1V_E_ARG and a reason that names the limit, in front of everything it would queue: nothing is launched, no
 * counter set is taken, and the next call on the encoder is an ordinary one.  A longer sequence is encoded in several calls (first_frame_index carries the position).  The
 * two to-bytes calls, m1v_convert_device and m1v_synth_device are not bound by it: they split their grids themselves. */
int m1v_create(m1v_encoder **out, int device, int width, int height, int channels,
               int quality_factor, int mode, int max_frames);
int m1v_batch_limit(const m1v_encoder *enc); /* the most frames one call may carry: min(max_frames, grid y, grid z extent) */
void m1v_destroy(m1v_encoder *enc);

/* Scratch policy.  Every run of 256 blocks owns a compact slot (what the kernel's LDS image of its bits can hold: 2 KiB at
 * quality <= 25); runs that emit more build their bits in a worst-case sized slot (28 KiB) taken from an overflow arena.  By
 * default the arena holds 1/256 of the runs — about 4x the payload in total at quality 12, where round 1 reserved 47x.
 * A batch that exhausts it reports M1V_STATUS_SCRATCH in its status word (its output is then undefined):
 * m1v_reserve_scratch(enc, 1) sizes the arena for every run (no batch can exhaust that), 0 returns to the default.
 * Both reallocate: call them between batches. */
int m1v_reserve_scratch(m1v_encoder *enc, int worst_case);
size_t m1v_scratch_bytes(const m1v_encoder *enc); /* device bytes currently held as scratch */

/* geometry helpers */
int m1v_strips(const m1v_encoder *enc);          /* x_extent / 16 */
int m1v_mb_rows(const m1v_encoder *enc);         /* y_extent / 16 */
size_t m1v_frame_bound(const m1v_encoder *enc);  /* worst-case bytes of one frame record */
size_t m1v_frame_bound_for(int width, int height, int mode); /* the same without an encoder (0: geometry not encodable) */
size_t m1v_frame_bytes_in(const m1v_encoder *enc); /* width*height*channels */

/* PACK(12)+SYS(15), written once per file.  Returns 27. */
size_t m1v_file_prolog(uint8_t out[27]);

/* n_frames frames, contiguous in d_rgb (interleaved, width*height*channels bytes each; or laid out as m1v_set_input_layout says), to
 * contiguous frame records in d_out.  first_frame_index is the global index of frame 0 of the batch
 * (it drives the `hour` fields, encoder.h:42,475-484).  d_rgb is only read, but a kernel may read up to the next
 * 4-byte boundary past a row's last byte (three bytes at most, inside the aligned word that holds that byte; pictures
 * whose width is not a multiple of 8 in a 4-byte aligned buffer): allocations are at least 4-byte granular, so this
 * never leaves the buffer's last word.
 *   d_frame_sizes  uint64[n_frames] bytes of each record (may be NULL)
 *   d_total        uint64[1] total bytes written (may be NULL)
 *   d_status       uint32[1] OR of M1V_STATUS_* (may be NULL; M1V_STATUS_SCRATCH: see m1v_reserve_scratch) */
int m1v_encode_device(m1v_encoder *enc, const uint8_t *d_rgb, int n_frames, int first_frame_index,
                      uint8_t *d_out, size_t out_cap, uint64_t *d_frame_sizes, uint64_t *d_total,
                      uint32_t *d_status, void *stream);

/* Per-frame quality factors and frame-size budgets.  A frame record depends only on the frame's pixels, its global index and
 * its quality factor, so every frame of a batch may have its own.  Contract: 1 <= q[f] <= the encoder's quality factor
 * (clamped to 1..100); every plan the encoder made for its own quality stays valid for coarser ones.  An entry of 0 or above
 * that bound sets M1V_STATUS_QUALITY in d_status, and the batch's output is undefined.  All three are calls like
 * m1v_encode_device (asynchronous on `stream`, same counter hand-over, pipelined mode included) and may be interleaved with it.
 *
 * m1v_encode_quality_device   m1v_encode_device with frame f at quality d_quality[f] (uint8[n_frames] on the device; NULL =
 *                             the encoder's quality for every frame, the plain call).
 * m1v_frame_sizes_device      the exact record size each frame would have at d_quality (NULL = the encoder's quality) into
 *                             d_frame_sizes, and the status bits of the encode into d_status; assembles nothing and writes
 *                             nothing else (no output buffer).  Costs the encode kernel of a plain call.
 * m1v_encode_budget_device    fit each frame into a byte budget with no host wait: probes the record size of every frame at each
 *                             of the n_candidates qualities in `candidates` (a HOST array, 1 <= K <= 8, strictly increasing, each
 *                             <= the encoder's quality), picks per frame the LARGEST candidate whose record fits the frame's
 *                             budget (the whole record, as d_frame_sizes counts it), or the smallest candidate and
 *                             M1V_STATUS_OVER_BUDGET when none fits, then encodes once at the picked qualities.  The budget of
 *                             frame f is d_max_frame_bytes[f] (uint64[n_frames] on the device) or, when that is NULL,
 *                             max_frame_bytes.  d_chosen (uint8[n_frames] on the device, may be NULL) receives the picks.
 *                             The candidates' sizes come from m1v_frame_size_table_device: where the table is fused
 *                             (m1v_size_table_fused: 3-channel tile encoders and 4-channel encoders) one size-table pass, then
 *                             the encode (about 3 plain encode kernels at K = 8); otherwise (only an encoder whose
 *                             path, input mode or run length a m1v_debug_set_* hook has forced) K probes + the encode, K + 1
 *                             encode kernels.  A probe that exhausts the overflow scratch reports M1V_STATUS_SCRATCH (probes
 *                             only: the fused table uses no scratch).
 * m1v_frame_size_table_device the exact record size of every frame at each of n_qualities qualities (a HOST array, 1..8 entries,
 *                             strictly increasing, each <= the encoder's quality): d_sizes[k * n_frames + f] (uint64, on the
 *                             device) is what m1v_frame_sizes_device returns for frame f at the uniform quality qualities[k].
 *                             d_status[k] (uint32[n_qualities], may be NULL) receives the status bits of quality k
 *                             (M1V_STATUS_UNENCODABLE: some block cannot be coded at qualities[k], whose sizes are then
 *                             undefined).  Nothing else is written.  ONE pass of a fused kernel (pixel stage once, quantise
 *                             and count per quality; no scratch, so never M1V_STATUS_SCRATCH) for 3-channel encoders on the tile
 *                             path and for every 4-channel encoder, whose encodes stay on the run kernels; one probe per
 *                             quality only for an encoder forced by a m1v_debug_set_* hook (3 channels forced to runs; 4
 *                             channels with a forced path, input mode or run length).  m1v_size_table_fused tells which.
 *                             n_frames == 0 writes nothing.
 * m1v_encode_batch_budget_device   fit the whole batch into batch_bytes (the sum of its records, d_total) with no host wait.
 *                             Candidates as for m1v_encode_budget_device; s[k][f] = the record size of frame f at candidate k
 *                             and T[k] = sum over f of s[k][f].  With top = the LARGEST k with T[k] <= batch_bytes: none ->
 *                             every frame at candidates[0] and M1V_STATUS_OVER_BUDGET; top = K - 1 -> every frame there;
 *                             otherwise every frame at candidate top or top + 1: with d[f] = s[top + 1][f] - s[top][f]
 *                             (signed), every frame with d[f] <= 0 goes up, then the frames with d[f] > 0 in the order of
 *                             (d[f], f) ascending, the longest prefix of that order whose d sum to at most the bytes left.
 *                             Without M1V_STATUS_OVER_BUDGET the total is at most batch_bytes.
 * m1v_encode_cbr_device       a constant bitrate: bytes_per_frame (r >= 1) per frame interval into a buffer of buffer_bytes
 *                             (C, r <= C < 2^62).  The level L (int64, bytes available to the next frame) starts at
 *                             min(*d_level_in, C); per frame in order the LARGEST candidate whose record is at most L is
 *                             picked, or candidates[0] and M1V_STATUS_OVER_BUDGET when none is, and L = min(C, L - record + r)
 *                             (it may go negative: the debt is repaid by later refills; a stream may owe less than 2^62
 *                             bytes).  The final L goes to *d_level_out (int64 on the device; may be d_level_in).  A call
 *                             that passes the previous call's d_level_out as d_level_in continues its stream: the result is
 *                             that of one call over the concatenated frames, and the host never reads the level.  Separate
 *                             pointers let a failed or M1V_STATUS_SCRATCH call be repeated from the same level.  n_frames
 *                             == 0 writes *d_total = 0, *d_status = 0 and *d_level_out = min(*d_level_in, C).
 *                             Both: d_chosen (uint8[n_frames] on the device, may be NULL) receives the picked qualities.  A
 *                             rule assumes nothing about how size grows with quality (but "the largest that fits" assumes that
 *                             the larger quality is the better picture: see m1v_encode_rd_device).  The headers are those of every other
 *                             call (the rule limits bytes; it signals nothing in the stream), and every record is that of the
 *                             frame at its picked quality.  One size table (m1v_frame_size_table_device), one pick kernel
 *                             (a single workgroup, k_rate_pick) and one encode, all on `stream`: the cost of
 *                             m1v_encode_budget_device with the same candidates plus that launch (17 us for the batch form,
 *                             28 us for the bitrate form at 300 frames, K = 8).  M1V_STATUS_SCRATCH of a probe (hook-forced
 *                             encoders only) passes on as there.
 * Argument errors (bad candidates or qualities, n_frames > max_frames, null pointers; for the bitrate: a null level pointer,
 * bytes_per_frame == 0, buffer_bytes < bytes_per_frame or buffer_bytes >= 2^62) return M1V_E_ARG before anything is launched.
 * Profiling (m1v_profile_*) counts one fused size-table pass as ONE launch of the dominant kernel: a budget, batch-budget or
 * bitrate call with K candidates reports 2 launches where m1v_size_table_fused is 1, K + 1 on a hook-forced encoder.
 *
 * m1v_size_table_fused        what a size table costs on this encoder, before a caller sizes K: 1 = one fused pass (about two
 *                             plain encode kernels at K = 8), 0 = one probe (one encode kernel) per quality, -1 = null. */
int m1v_size_table_fused(const m1v_encoder *enc);
int m1v_encode_quality_device(m1v_encoder *enc, const uint8_t *d_rgb, int n_frames, int first_frame_index,
                              const uint8_t *d_quality, uint8_t *d_out, size_t out_cap, uint64_t *d_frame_sizes,
                              uint64_t *d_total, uint32_t *d_status, void *stream);
int m1v_frame_sizes_device(m1v_encoder *enc, const uint8_t *d_rgb, int n_frames, const uint8_t *d_quality,
                           uint64_t *d_frame_sizes, uint32_t *d_status, void *stream);
int m1v_encode_budget_device(m1v_encoder *enc, const uint8_t *d_rgb, int n_frames, int first_frame_index,
                             const uint8_t *candidates, int n_candidates, uint64_t max_frame_bytes,
                             const uint64_t *d_max_frame_bytes, uint8_t *d_chosen,
                             uint8_t *d_out, size_t out_cap, uint64_t *d_frame_sizes, uint64_t *d_total,
                             uint32_t *d_status, void *stream);
int m1v_frame_size_table_device(m1v_encoder *enc, const uint8_t *d_rgb, int n_frames, const uint8_t *qualities, int n_qualities,
                                uint64_t *d_sizes, uint32_t *d_status, void *stream);
int m1v_encode_batch_budget_device(m1v_encoder *enc, const uint8_t *d_rgb, int n_frames, int first_frame_index,
                                   const uint8_t *candidates, int n_candidates, uint64_t batch_bytes, uint8_t *d_chosen,
                                   uint8_t *d_out, size_t out_cap, uint64_t *d_frame_sizes, uint64_t *d_total,
                                   uint32_t *d_status, void *stream);
int m1v_encode_cbr_device(m1v_encoder *enc, const uint8_t *d_rgb, int n_frames, int first_frame_index,
                          const uint8_t *candidates, int n_candidates, uint64_t bytes_per_frame, uint64_t buffer_bytes,
                          const int64_t *d_level_in, int64_t *d_level_out, uint8_t *d_chosen,
                          uint8_t *d_out, size_t out_cap, uint64_t *d_frame_sizes, uint64_t *d_total,
                          uint32_t *d_status, void *stream);

/* Distortion and rate-distortion picks.  The byte rules above take the LARGEST candidate that fits, which assumes that a larger
 * quality factor gives a better picture.  In this encoder it need not: VLC_encode codes the AC levels of a block only up to the
 * first non-zero level whose predecessor is non-zero too and drops the rest, and a finer quantiser makes that stop come earlier
 * ("Distortion and rate-distortion picks": a smooth gradient loses 15 times more at quality 92 than at 38).  These two
 * calls tell the caller, and pick by it.
 *
 * The measure, an exact integer.  For one block at one quality: c[p] the 64 unquantised coefficients in zigzag position (the
 * reference's fast_DCT), d[p] the quality's divisors (scale_quantization_matrix), l[p] = c[p] / d[p] by C's truncating division
 * (quantization), E = position 0 and the AC positions the record codes (the non-zero l[p], p >= 1, below the first p >= 1 with
 * l[p] != 0 and l[p - 1] != 0):
 *     D(block) = sum over p in E of (c[p] - l[p] * d[p])^2  +  sum over p not in E of c[p]^2
 * and D(frame, quality) is the sum over every block the macroblock loops visit.  It is the squared error, in the reference's
 * coefficient domain, between what the encoder transformed and what the record carries; that FDCT is scaled like the orthonormal
 * one (DC = sum of the pixels / 8), so D tracks the squared error in the pixel domain.  An encoder-side measure: the library
 * decodes nothing.
 *
 * m1v_frame_rd_table_device   m1v_frame_size_table_device plus the distortion: d_sizes[k * n_frames + f] is exactly what that call
 *                             writes, d_distortion[k * n_frames + f] (uint64, on the device) = D(frame f, qualities[k]).
 *                             d_status[k] as there (may be NULL); with M1V_STATUS_UNENCODABLE at k both rows of k are undefined,
 *                             the other rows stay exact.  Qualities are checked as there; every input layout in force is
 *                             served (packed 3 and 4 channels, surface, planes).  ONE pass of a fused kernel (the k_rd_table_*
 *                             kernels: the size-table pass with a second sweep over the block's coefficients per quality; cost
 *                             beside the size table: not measured yet, tools/rd_table_timing.py), on `stream`, no scratch, in
 *                             pipelined mode too; m1v_profile_* counts it as one launch.  n_frames == 0 writes nothing.  An
 *                             encoder whose size table is not fused (m1v_size_table_fused == 0: hook-forced only) returns
 *                             M1V_E_ARG: there is no probe fallback for the distortion.  m1v_debug_fail_encode reaches its
 *                             stages as those of the size table.
 * m1v_encode_rd_device        one rd table over `candidates` (as m1v_encode_budget_device's), one pick kernel (k_rd_pick, a lane
 *                             per frame) and one encode at the picked per-frame qualities, all on `stream` with no host wait.
 *                             The limit of frame f is d_limits[f] (uint64[n_frames] on the device) or, when that is NULL, `limit`.
 *                             A candidate whose table status carries M1V_STATUS_UNENCODABLE is out of the running for every
 *                             frame; with every candidate out each frame goes to candidates[0] and the encode reports the bit.
 *                             Among the others, with s = the record size and D = the distortion of the frame at a candidate:
 *     M1V_RD_BEST_IN_BUDGET            of those with s <= limit the least D (ties: the smaller record, then the smaller k); if none
 *                                      fits, the smallest record (ties: the smaller k) and M1V_STATUS_OVER_BUDGET.
 *     M1V_RD_SMALLEST_AT_DISTORTION    of those with D <= limit the smallest record (ties: the less D, then the smaller k); if none
 *                                      qualifies, the least D (ties: the smaller record, then the smaller k) and
 *                                      M1V_STATUS_OVER_DISTORTION (output valid).
 *                             d_chosen (uint8[n_frames]) and d_frame_distortion (uint64[n_frames], the picked candidate's D) may
 *                             be NULL; the other outputs are m1v_encode_device's, and every record is that of the frame at its
 *                             picked quality.  M1V_E_ARG before anything is launched: an unknown rule, bad candidates, n_frames >
 *                             max_frames, a null d_rgb or d_out, an encoder whose size table is not fused.  A profiled call
 *                             reports 2 launches. */
enum { M1V_RD_BEST_IN_BUDGET = 0, M1V_RD_SMALLEST_AT_DISTORTION = 1 };
enum { M1V_STATUS_OVER_DISTORTION = 32u };
int m1v_frame_rd_table_device(m1v_encoder *enc, const uint8_t *d_rgb, int n_frames, const uint8_t *qualities, int n_qualities,
                              uint64_t *d_sizes, uint64_t *d_distortion, uint32_t *d_status, void *stream);
int m1v_encode_rd_device(m1v_encoder *enc, const uint8_t *d_rgb, int n_frames, int first_frame_index,
                         const uint8_t *candidates, int n_candidates, int rule, uint64_t limit, const uint64_t *d_limits,
                         uint8_t *d_chosen, uint8_t *d_out, size_t out_cap, uint64_t *d_frame_sizes,
                         uint64_t *d_frame_distortion, uint64_t *d_total, uint32_t *d_status, void *stream);

/* Batch budgets and constant bitrate that pick by distortion: "this batch in B bytes" and "this stream at r bytes per frame" by
 * the rd table instead of by "the largest quality that fits", with no host wait.  The table is the rd table's: s[k][f] record
 * bytes and D[k][f] distortion of frame f at candidate k.
 *
 * A candidate whose table status carries M1V_STATUS_UNENCODABLE is out of the running for every frame.  With every candidate out,
 * each frame goes to candidate 0 (candidate 0 alone is then in the running) and the encode reports the bit.
 *
 * The chain of a frame is the lower convex hull of its (s, D) points, walked from the smallest record towards less distortion:
 *   - v0 = the candidate with the least s.  Ties go to the less D, then the smaller k.
 *   - From vertex v, the next vertex is, among candidates with s > s[v] and D < D[v], the one with the greatest
 *     (D[v] - D) / (s - s[v]).
 *   - Ratios are compared exactly, by cross products in 128 bits.
 *   - Ties go to the smaller s, then the smaller k.
 *   - The chain ends when no such candidate exists.
 * Step j >= 1 of frame f has ds > 0 bytes and dd > 0 distortion gained.  Along a chain dd / ds never increases.
 *
 * The order of all steps of a batch: dd / ds descending (exact cross products).  Ties go by frame ascending, then j ascending.
 *
 * Batch form, M1V_RD_BEST_IN_BUDGET, limit = bytes for the sum of the records.
 *   - Every frame starts at its v0.
 *   - If those records sum to more than the limit, every frame stays at v0 and the status is M1V_STATUS_OVER_BUDGET.
 *   - Otherwise the steps are taken in that order: the longest prefix whose ds sum to at most the bytes left.  Every ds is
 *     positive, so a step is taken iff its own inclusive prefix sum fits.
 *   - A frame ends at the vertex its last taken step reaches.
 *   - Without the status bit, the total is at most the limit.
 * Batch form, M1V_RD_SMALLEST_AT_DISTORTION, limit = ceiling for the sum of the frames' D.
 *   - Same start and same order.
 *   - The shortest prefix after which the sum of D is at most the limit is taken.  That is none if the start already qualifies.
 *   - If even every step does not reach the limit, every frame is at its chain's end and the status is
 *     M1V_STATUS_OVER_DISTORTION.  The output is valid.
 * Bitrate form.
 *   - It is the leaky bucket of m1v_encode_cbr_device, unchanged: level, refill, capacity, d_level_in / d_level_out, chaining,
 *     and debts.
 *   - Per frame, the pick is M1V_RD_BEST_IN_BUDGET with the level as the limit.  That is the least D among records <= level,
 *     with ties to the smaller record, then the smaller k.
 *   - If nothing fits, the frame takes the smallest record, with ties to the smaller k, and the status is
 *     M1V_STATUS_OVER_BUDGET.
 *
 * The batch forms are the Lagrangian greedy on each frame's hull, NOT the knapsack optimum: a prefix of the steps by slope is the
 * best allocation for the bytes it uses, but the bytes left behind the last step that fits are not spent on a cheaper step
 * further down.  On random 4 x 5 tables a CPU prototype stayed within 1 % of the exhaustive optimum's distortion on average; the
 * worst case was 29 %.
 *
 * m1v_encode_rd_batch_device  m1v_encode_rd_device with the batch pick: the same checks in the same order, one rd table into the
 *                             encoder's own tables, the pick (k_rd_chains, a lane per frame, then k_rd_batch_pick, a lane per
 *                             step over a grid of workgroups) and one encode at the picked qualities, all on `stream`, in
 *                             pipelined mode too.  Every input layout is served.  d_chosen and d_frame_distortion may be NULL.
 *                             A profiled call reports 2 launches.  Cost at 300 x 1080p, K = 8: 1.19 x m1v_encode_rd_device
 *                             (the pick takes 0.44 ms; profiles/r15_rd_rate_timing.txt), the bitrate form 1.01 x.
 * m1v_encode_rd_cbr_device    m1v_encode_cbr_device with the bitrate pick above (k_rd_cbr_pick, one workgroup): its arguments
 *                             and their checks, then "not fused" as m1v_encode_rd_device.
 *                             Both: n_frames == 0 writes *d_total = 0 and *d_status = 0 (the bitrate form also *d_level_out =
 *                             min(*d_level_in, C)) and nothing else.  m1v_debug_fail_encode reaches the table's and the
 *                             encode's stages as in m1v_encode_rd_device.
 * m1v_rd_batch_pick_device, m1v_rd_cbr_pick_device
 *                             the pick alone, on a table the caller holds on the device in m1v_frame_rd_table_device's layout
 *                             ([k * n_frames + f]; d_table_status uint32[n_candidates], may be NULL: every candidate in the
 *                             running): re-pick at another limit without another table pass.  d_picks (uint8[n_frames]) receives
 *                             the candidate INDEX of every frame, d_pick_distortion (uint64[n_frames], may be NULL) its D,
 *                             d_status (uint32[1]) the status word, WRITTEN, not OR'ed; the bitrate form moves the level as the
 *                             encode does.  Only the pick is launched (the batch form uses the encoder's step table: calls on
 *                             one encoder are ordered by the stream).  Needs n_frames <= max_frames, 1 <= n_candidates <= 8 and
 *                             non-null tables, picks and status (the bitrate form: level pointers and rates as
 *                             m1v_encode_cbr_device); M1V_E_ARG before anything is launched otherwise.  Preconditions (the
 *                             library's own tables meet them): every s < 2^32 and every D < 2^63.  A table outside that gives
 *                             unspecified picks but no access outside the arrays.  n_frames == 0 writes *d_status = 0 (the
 *                             bitrate form also the level) and nothing else. */
int m1v_encode_rd_batch_device(m1v_encoder *enc, const uint8_t *d_rgb, int n_frames, int first_frame_index,
                               const uint8_t *candidates, int n_candidates, int rule, uint64_t limit, uint8_t *d_chosen,
                               uint8_t *d_out, size_t out_cap, uint64_t *d_frame_sizes, uint64_t *d_frame_distortion,
                               uint64_t *d_total, uint32_t *d_status, void *stream);
int m1v_encode_rd_cbr_device(m1v_encoder *enc, const uint8_t *d_rgb, int n_frames, int first_frame_index,
                             const uint8_t *candidates, int n_candidates, uint64_t bytes_per_frame, uint64_t buffer_bytes,
                             const int64_t *d_level_in, int64_t *d_level_out, uint8_t *d_chosen,
                             uint8_t *d_out, size_t out_cap, uint64_t *d_frame_sizes, uint64_t *d_frame_distortion,
                             uint64_t *d_total, uint32_t *d_status, void *stream);
int m1v_rd_batch_pick_device(m1v_encoder *enc, const uint64_t *d_sizes, const uint64_t *d_distortion, const uint32_t *d_table_status,
                             int n_frames, int n_candidates, int rule, uint64_t limit, uint8_t *d_picks,
                             uint64_t *d_pick_distortion, uint32_t *d_status, void *stream);
int m1v_rd_cbr_pick_device(m1v_encoder *enc, const uint64_t *d_sizes, const uint64_t *d_distortion, const uint32_t *d_table_status,
                           int n_frames, int n_candidates, uint64_t bytes_per_frame, uint64_t buffer_bytes,
                           const int64_t *d_level_in, int64_t *d_level_out, uint8_t *d_picks, uint64_t *d_pick_distortion,
                           uint32_t *d_status, void *stream);

/* Streams: many in one batch.  Every call above takes one first_frame_index (frame f of the batch is frame first_frame_index + f
 * of ONE stream), and the bitrate calls keep one leaky bucket.  No single stream feeds this encoder; a deployment mixes tens or
 * hundreds, a few frames each per step.  These calls take a batch that is the concatenation of n_streams spans,
 * 1 <= n_streams <= M1V_MAX_STREAMS:
 *
 *   d_rgb          exactly what it is for m1v_encode_device under the layout and table mode in force.  Span s covers batch
 *                  positions [first_frame, first_frame + n_frames); with a frame table or plane table the caller orders the
 *                  entries stream by stream at no cost.
 *   the index      frame first_frame + j of span s is frame first_frame_index + j of its stream.
 *   the record     byte for byte what m1v_encode_quality_device gives for that frame alone, at that index and quality.
 *   the output     records lie in d_out in batch order, so each stream's records are one contiguous range;
 *                  d_stream_bytes[s] (uint64[n_streams] on the device, may be NULL) is the length of that range.  A span of 0
 *                  frames writes 0.
 *
 * The spans (d_spans, m1v_stream_span[n_streams]) live on the DEVICE and are read only by kernels, on `stream`, as a frame table
 * is: a caller may build them with work queued in front of the call.  The host cannot validate them, so the device does.  The
 * spans must tile the batch in order: first_frame of span 0 is 0; first_frame of span s + 1 is first_frame + n_frames of span s;
 * the last span ends at the call's n_frames.  Anything else sets M1V_STATUS_STREAMS in d_status, and the batch's output is then
 * undefined, as it is for M1V_STATUS_QUALITY.  Every index derived from a span is clamped into [0, n_frames] before it addresses
 * anything: bad spans give unspecified records and never an access outside the arrays.  M1V_E_ARG before anything is launched:
 * null spans, n_streams outside 1 .. M1V_MAX_STREAMS, a spans pointer that is not 4-byte aligned, and everything the plain calls
 * check.
 *
 * m1v_encode_streams_device   m1v_encode_quality_device (d_quality may be NULL: the encoder's quality) with the indices taken from
 *                             the spans.  n_frames == 0 writes *d_total = 0, *d_status = 0 and zeros into d_stream_bytes.
 *                             Kernels: k_streams_map (a lane per span) in front of the encode kernel checks the tiling and
 *                             expands the spans into a per-frame index array of the encoder (one per counter set: in pipelined
 *                             mode both batches in flight keep theirs); k_assemble runs as in every other call, with index 0;
 *                             k_streams_finish behind it, on the stream k_assemble runs on, rewrites the 44 header bytes of every
 *                             record that fitted d_out (all but the packet length) from the frame's own index and sums each
 *                             span's records.  Cost beside m1v_encode_device with one span: 1.03 x at 300 x 1080p, 1.01 x at
 *                             100 x 4K (16 and 9 us; the A/A spread is 0.98 .. 1.12; profiles/r26_streams_timing.txt).
 * m1v_encode_streams_cbr_device   a constant bitrate with one leaky bucket per stream: the arguments of m1v_encode_cbr_device
 *                             with the spans in place of first_frame_index.  The bucket of stream s is the existing one,
 *                             unchanged: it starts at min(d_level_in[s], C_s) and walks the span's frames in order with
 *                             L = min(C_s, L - record + r_s); the final L goes to d_level_out[s] (int64[n_streams] each; they
 *                             may alias elementwise).  Streams do not interact.  `rule` selects the pick:
 *     M1V_STREAMS_LARGEST_THAT_FITS   m1v_encode_cbr_device's pick, on one size table.
 *     M1V_STREAMS_LEAST_DISTORTION    m1v_encode_rd_cbr_device's pick, on one rd table (unencodable candidates are out of the
 *                                     running, as they are there).
 *                             d_stream_rates (m1v_stream_rate[n_streams] on the device) holds r_s and C_s; NULL means
 *                             bytes_per_frame and buffer_bytes apply to every stream, host-checked as in m1v_encode_cbr_device.
 *                             A device entry outside 1 <= r <= C < 2^62 sets M1V_STATUS_STREAMS; its stream's frames go to
 *                             candidate 0 and its level passes through unchanged.  M1V_STATUS_OVER_BUDGET is set if any stream
 *                             found a frame that nothing fits.  An empty span writes d_level_out[s] = min(d_level_in[s], C_s).
 *                             d_chosen, d_frame_distortion (written under the distortion rule) and d_stream_bytes may be NULL.
 *                             One table pass, one pick launch (k_streams_bitrate, one wave per stream over a grid of
 *                             workgroups) and one encode for the whole batch, with no host wait, in pipelined mode too.  An
 *                             encoder whose tables are not fused behaves as in the two existing bitrate calls (the distortion
 *                             rule returns M1V_E_ARG).  Cost at K = 8 (tools/streams_timing.py, profiles/r26_streams_timing.txt):
 *                             30 streams x 10 frames of 1080p take 0.59 of the time of one existing bitrate call per stream
 *                             (either rule; 20 x 5 frames of 4K: 0.74 and 0.73), and 1.02 / 1.00 of ONE existing call over
 *                             the 300 frames behind one bucket (byte rule / distortion rule).
 * m1v_streams_cbr_pick_device the pick alone on a table the caller holds: the streams form of m1v_rd_cbr_pick_device, with the same
 *                             table layout, preconditions and WRITTEN, not OR'ed, status.  d_distortion may be NULL under the
 *                             byte rule (d_pick_distortion is then not written).  Bad spans set M1V_STATUS_STREAMS here too.
 *
 * Not covered: m1v_delivery_step (and the CLI) with spans; the host-buffer entry points.  A byte budget or a distortion ceiling
 * per stream: "Streams: a budget per stream", below. */
typedef struct m1v_stream_span {
    uint32_t first_frame;        /* position in the batch of the span's first frame          */
    uint32_t n_frames;           /* frames of this stream in the batch; 0 is allowed         */
    int32_t  first_frame_index;  /* global index, in ITS stream, of the span's first frame   */
    uint32_t reserved;           /* 0                                                        */
} m1v_stream_span;               /* 16 bytes; the array lives on the DEVICE                  */
typedef struct m1v_stream_rate {
    uint64_t bytes_per_frame;    /* r_s: 1 <= r_s <= C_s                                     */
    uint64_t buffer_bytes;       /* C_s < 2^62                                               */
} m1v_stream_rate;               /* 16 bytes; the array lives on the DEVICE                  */
enum { M1V_STATUS_STREAMS = 64u };
enum { M1V_MAX_STREAMS = 4096 };
enum { M1V_STREAMS_LARGEST_THAT_FITS = 0, M1V_STREAMS_LEAST_DISTORTION = 1 };
int m1v_encode_streams_device(m1v_encoder *enc, const uint8_t *d_rgb, int n_frames, const m1v_stream_span *d_spans, int n_streams,
                              const uint8_t *d_quality, uint8_t *d_out, size_t out_cap, uint64_t *d_frame_sizes,
                              uint64_t *d_stream_bytes, uint64_t *d_total, uint32_t *d_status, void *stream);
int m1v_encode_streams_cbr_device(m1v_encoder *enc, const uint8_t *d_rgb, int n_frames, const m1v_stream_span *d_spans, int n_streams,
                                  const uint8_t *candidates, int n_candidates, int rule, uint64_t bytes_per_frame,
                                  uint64_t buffer_bytes, const m1v_stream_rate *d_stream_rates, const int64_t *d_level_in,
                                  int64_t *d_level_out, uint8_t *d_chosen, uint8_t *d_out, size_t out_cap, uint64_t *d_frame_sizes,
                                  uint64_t *d_frame_distortion, uint64_t *d_stream_bytes, uint64_t *d_total, uint32_t *d_status,
                                  void *stream);
int m1v_streams_cbr_pick_device(m1v_encoder *enc, const uint64_t *d_sizes, const uint64_t *d_distortion, const uint32_t *d_table_status,
                                int n_frames, int n_candidates, const m1v_stream_span *d_spans, int n_streams, int rule,
                                uint64_t bytes_per_frame, uint64_t buffer_bytes, const m1v_stream_rate *d_stream_rates,
                                const int64_t *d_level_in, int64_t *d_level_out, uint8_t *d_picks, uint64_t *d_pick_distortion,
                                uint32_t *d_status, void *stream);

/* Streams: a budget per stream.  The batch rules above ("these frames in B bytes", "these frames under a distortion ceiling")
 * with one limit per stream of a batch of many streams, in one call.
 *
 * The batch is the concatenation of n_streams spans.
 *   - The spans are those of m1v_encode_streams_device: on the device, validated and clamped there, M1V_STATUS_STREAMS otherwise.
 *   - Stream s has the limit L_s = d_stream_limits[s] (uint64[n_streams] on the device, 8-byte aligned).
 *   - With d_stream_limits NULL, L_s = `limit` for every stream.
 * Streams do not interact.
 *   - The picks of the frames of span s are exactly what the single-batch rule gives on the sub-table of that span's frames
 *     alone, with the limit L_s.
 *   - `rule` names the single-batch rule and the bit a stream over its limit sets:
 *       M1V_SPANS_LARGEST_THAT_FITS       m1v_encode_batch_budget_device's                               M1V_STATUS_OVER_BUDGET
 *       M1V_SPANS_LEAST_DISTORTION        m1v_rd_batch_pick_device's, M1V_RD_BEST_IN_BUDGET             M1V_STATUS_OVER_BUDGET
 *       M1V_SPANS_SMALLEST_AT_DISTORTION  m1v_rd_batch_pick_device's, M1V_RD_SMALLEST_AT_DISTORTION     M1V_STATUS_OVER_DISTORTION
 *   - "Frame ascending" in every tie rule is position in the batch.  Inside one span that is position in the span.
 *   - Candidates whose table status carries M1V_STATUS_UNENCODABLE are treated as the single-batch rule treats them.
 *   - An empty span picks nothing and is not over.
 * The status words.
 *   - d_stream_status[s] (uint32[n_streams] on the device, may be NULL) receives stream s's over bit, or 0.
 *   - The batch's status word receives the OR over the streams.
 *   - It receives M1V_STATUS_STREAMS for spans that do not tile the batch.
 *   - It receives whatever the single-batch call passes on (M1V_STATUS_SCRATCH of the table).
 * Bad spans.
 *   - The picks are unspecified, but every frame's pick is a candidate index below n_candidates.
 *   - A frame that no clamped span covers takes candidate 0.
 *   - Nothing outside the arrays is touched.
 * Preconditions of the pick-only call: those of m1v_rd_batch_pick_device, every s < 2^32 and every D < 2^63.  Sums of
 * distortions are taken in 128 bits.
 *
 * m1v_encode_streams_budget_device
 *   - One table pass: the size table under M1V_SPANS_LARGEST_THAT_FITS, the rd table under the other two rules.
 *   - One pick: k_span_plan, k_rd_chains under the two rules that pick by distortion, k_span_budget.
 *   - One encode at the picked per-frame qualities, and k_streams_finish for the indices and d_stream_bytes.
 *   - All of it on `stream`, with no host wait, in pipelined mode too.  Every input layout and both tables are served.
 *   - The argument checks are m1v_encode_streams_cbr_device's, in its order, then an unknown rule and a d_stream_limits that
 *     is not 8-byte aligned: M1V_E_ARG before anything is launched.
 *   - On an encoder whose tables are not fused, the two rules that pick by distortion return M1V_E_ARG, as m1v_encode_rd_device
 *     does, and M1V_SPANS_LARGEST_THAT_FITS falls back to probes, as m1v_encode_batch_budget_device does.
 *   - d_chosen, d_frame_distortion, d_stream_bytes and d_stream_status may be NULL.  d_frame_distortion is written under the
 *     two rules that pick by distortion.
 *   - n_frames == 0 writes *d_total = 0, *d_status = 0 and zeros into d_stream_bytes and d_stream_status.
 *   - m1v_debug_fail_encode reaches the table's and the encode's stages as in m1v_encode_streams_cbr_device.
 *   - A profiled call reports 2 launches.
 * m1v_streams_budget_pick_device
 *   - The pick alone on a table the caller holds: the streams form of m1v_rd_batch_pick_device, with the same table layout.
 *   - d_picks receives candidate INDICES.  d_status is WRITTEN, not OR'ed.
 *   - d_distortion may be NULL under M1V_SPANS_LARGEST_THAT_FITS; d_pick_distortion is then not written.
 *   - It uses the encoder's step table and span prefix: calls on one encoder are ordered by the stream.
 *   - n_frames == 0 writes the status words (every span is empty) and no pick.
 * Kernels (csrc/m1v_span_budget.h).
 *   - k_span_plan, one workgroup: the exclusive prefix of max(1, ceil(n_s / 32)) over the clamped spans.
 *   - k_span_budget, n_streams + ceil(n_frames / 32) workgroups: workgroup w finds its span and its chunk of 32 frames in that
 *     prefix and compares its steps (its frames, under M1V_SPANS_LARGEST_THAT_FITS) with those of its own span only.
 *   - The compares cost the sum of n_s^2 over the streams, where k_rd_batch_pick costs n^2.
 * Cost at K = 8 (tools/streams_budget_timing.py, profiles/r33_streams_budget_timing.txt).
 *   - 30 streams x 10 frames of 1080p take 0.51 (by size) and 0.43 (by distortion) of the time of one existing batch call per
 *     stream; 20 x 5 frames of 4K take 0.69 and 0.59.
 *   - Against ONE existing batch call over all the frames with a single limit: 1.039 and 0.847 at 1080p, 1.022 and 0.957 at 4K.
 *   - The A/A range is 0.999 .. 1.027 at 1080p and 0.999 .. 1.004 at 4K: by size the call lies above it (60 and 47 us: the map,
 *     the plan and the finish are launches the single-limit call does not make); by distortion it is cheaper than one limit.
 *
 * Not covered: m1v_delivery_step (and the CLI) with spans; the host-buffer entry points. */
enum { M1V_SPANS_LARGEST_THAT_FITS = 0, M1V_SPANS_LEAST_DISTORTION = 1, M1V_SPANS_SMALLEST_AT_DISTORTION = 2 };
int m1v_encode_streams_budget_device(m1v_encoder *enc, const uint8_t *d_rgb, int n_frames, const m1v_stream_span *d_spans, int n_streams,
                                     const uint8_t *candidates, int n_candidates, int rule, uint64_t limit,
                                     const uint64_t *d_stream_limits, uint8_t *d_chosen, uint8_t *d_out, size_t out_cap,
                                     uint64_t *d_frame_sizes, uint64_t *d_frame_distortion, uint64_t *d_stream_bytes,
                                     uint32_t *d_stream_status, uint64_t *d_total, uint32_t *d_status, void *stream);
int m1v_streams_budget_pick_device(m1v_encoder *enc, const uint64_t *d_sizes, const uint64_t *d_distortion, const uint32_t *d_table_status,
                                   int n_frames, int n_candidates, const m1v_stream_span *d_spans, int n_streams, int rule,
                                   uint64_t limit, const uint64_t *d_stream_limits, uint8_t *d_picks, uint64_t *d_pick_distortion,
                                   uint32_t *d_stream_status, uint32_t *d_status, void *stream);

/* Input layout: frames that already live on the device as windows of pitched surfaces, in R,G,B(,A) or B,G,R(,A) byte order,
 * encoded where they lie (no compaction or swizzle copy in front of the encoder).
 *
 *   m1v_set_input_layout(enc, row_pitch_bytes, frame_stride_bytes, order)
 *
 * d_rgb of every *_device call then points at the first byte of the window's first pixel in frame 0; row y of frame f starts at
 * d_rgb + f * frame_stride + y * row_pitch.  Any byte alignment of the pointer, the pitch and the stride is accepted.  order is
 * the order of the three colour bytes of a pixel; a 4th byte is skipped.
 *   (0, 0, M1V_ORDER_RGB)   the DEFAULT layout: packed frames, served by exactly the kernels of an encoder whose layout was never
 *                           set.  Setting it again after a surface layout restores that plan (m1v_path_in_use is then 0 again
 *                           for 4 channels).
 *   anything else           a SURFACE layout, served by the surface kernels (k_encode_surface, k_size_table_surface: the tile
 *                           workgroup behind a pitched front half), also when the pitch equals width * channels: the same
 *                           packed buffer through both kernel families gives the same bytes (the A/B reference inside one
 *                           process, like the m1v_debug_set_* hooks), and a 4-channel caller opts into the tile-shaped encode
 *                           this way.  row_pitch 0 = width * channels; frame_stride 0 = height * row_pitch.
 * With a surface layout m1v_path_in_use and m1v_size_table_fused are 1 for 3 and 4 channels, and every *_device encode, probe,
 * size-table, budget, batch-budget and bitrate call, pipelined mode, m1v_reserve_scratch, m1v_debug_set_lds_words and
 * m1v_delivery_* work as on the tile path.  It is a reconfiguration like m1v_reserve_scratch: call it between batches; new
 * buffers are allocated first and swapped in on success, so a failed call (M1V_E_HIP) leaves the encoder as it was.
 * M1V_E_ARG, before anything is launched or reallocated: 0 < row_pitch < width * channels; 0 < frame_stride <
 * (height - 1) * row_pitch + width * channels; (height - 1) * row_pitch + width * channels >= 2^32 (offsets inside a frame are
 * 32-bit); an unknown order; a surface layout with an odd width (the reference addresses its chroma plane with stride width / 2:
 * with an odd width a chroma block row straddles two picture rows and is no run of bytes inside one pitched row; odd widths keep
 * working on the default layout); a surface layout on an encoder that a hook has forced to the run kernels (m1v_debug_set_path 0,
 * m1v_debug_set_input_mode, m1v_debug_set_dense_threads) — conversely those hooks return M1V_E_ARG on an encoder with a surface
 * layout.
 * Packed only: m1v_coefficients_device, m1v_convert_device, m1v_encode_host, m1v_encode_planes_host and m1v_convert_host return
 * M1V_E_ARG while a surface layout is set.
 * Read contract: of frame f a kernel reads only bytes of [d_rgb + f * frame_stride, d_rgb + f * frame_stride +
 * (height - 1) * row_pitch + width * channels), rounded up to the next 4-byte boundary as for packed input.  Padding bytes inside
 * that range (between a row's last pixel and the next row, a 4th byte of a pixel) may be read; they never influence the output.
 *
 *   m1v_input_layout(enc, &row_pitch, &frame_stride, &order)   the layout in force: (0, 0, M1V_ORDER_RGB) for the default, else
 *                           the pitch and the stride in bytes as the kernels use them (no zeros).  Any pointer may be NULL. */
enum { M1V_ORDER_RGB = 0, M1V_ORDER_BGR = 1 };   /* byte order of the three colour bytes of a pixel; a 4th byte is skipped */
int m1v_set_input_layout(m1v_encoder *enc, size_t row_pitch_bytes, size_t frame_stride_bytes, int order);
int m1v_input_layout(const m1v_encoder *enc, size_t *row_pitch_bytes, size_t *frame_stride_bytes, int *order);

/* Plane layout: frames that are already YCbCr in planes on the device — the output of m1v_convert_device, of a hardware video or
 * JPEG decoder (NV12), of a camera pipeline (I420) — encoded as they are: no colour conversion, and so no lossy
 * YCbCr -> RGB -> YCbCr round trip in front of the encoder.  For encoders created with channels = 3.
 *
 * Definition.  Frame f starts at F = d_rgb + f * frame_stride; the region coded is xe x ye = (m1v_strips * 16) x (m1v_mb_rows * 16).
 * The macroblock at (x, y) takes
 *     luma block k (Y0..Y3), row i            the 8 bytes at  F + y_offset + (y + 8 * (k / 2) + i) * y_pitch + x + 8 * (k % 2)
 *     chroma plane p (Cb, Cr), row i, sample j    the byte at  F + p_offset + (y / 2 + i) * c_pitch + (x / 2 + j) * c_step
 * and the record is what the reference's frame body makes of those bytes behind its colour conversion (encoder.h:238-444): the
 * same headers, first_frame_index, status bits, per-frame quality and sizes as the RGB calls.  The chroma formula is the
 * reference's own (it cuts chroma blocks from its full-resolution Cb / Cr planes addressed with stride width / 2,
 * encoder.h:347-348): with the planes m1v_convert_device writes and c_pitch = width / 2 the record IS the RGB record of the same
 * picture; with true 4:2:0 planes (width / 2 x height / 2 samples) the same formula is ordinary 4:2:0 sampling.
 * Any byte alignment of the pointer, the offsets, the pitches and the stride is accepted, and so are odd widths.  Planes may
 * overlap (NV12's do); they are only read.
 *
 *   m1v_plane_layout_preset(width, height, preset, &layout)   pure host arithmetic (no encoder, no device): tightly packed
 *     M1V_PLANES_REFERENCE   Y at 0, Cb at W*H, Cr at 2*W*H, pitches W and W/2, c_step 1, stride 3*W*H (m1v_convert_device's output)
 *     M1V_PLANES_I420 / _YV12   W*H luma, then two (W/2)*(H/2) planes in Cb,Cr / Cr,Cb order, c_pitch W/2, stride W*H*3/2
 *     M1V_PLANES_NV12 / _NV21   W*H luma, then one plane of interleaved Cb,Cr / Cr,Cb pairs: c_step 2, c_pitch W, the second
 *                               component's offset = the first's + 1, stride W*H*3/2
 *     The 4:2:0 presets need an even width and height (M1V_E_ARG otherwise); REFERENCE takes any.  M1V_E_ARG: unknown preset.
 *   m1v_set_plane_layout(enc, &layout)   NULL = back to the default layout.  A reconfiguration like m1v_set_input_layout (call it
 *     between batches; buffers are allocated first and swapped in on success).  The encoder takes the tile plan (m1v_path_in_use
 *     and m1v_size_table_fused are 1) behind the plane kernels (k_encode_planes, k_size_table_planes).  ONE input layout is in
 *     force at a time: a plane layout replaces a surface layout and the other way round; m1v_set_plane_layout(enc, NULL) and
 *     m1v_set_input_layout(enc, 0, 0, M1V_ORDER_RGB) both restore the default plan.  While a plane layout is in force
 *     m1v_input_layout returns M1V_E_ARG.  Every *_device encode, probe, size-table, budget, batch-budget and bitrate call,
 *     pipelined mode, m1v_reserve_scratch, m1v_debug_set_lds_words, m1v_delivery_* and the m1v_profile_* counters work on it.
 *     M1V_E_ARG, before anything is launched or reallocated: a null encoder; channels != 3; c_step > 2; frame_stride 0;
 *     0 < y_pitch < width; 0 < c_pitch < (width / 2) * c_step; a frame extent E (below) of 2^32 or more; frame_stride < E; an
 *     encoder that a hook has forced to the run kernels (those hooks return M1V_E_ARG on an encoder with a plane layout).
 *     Packed only: m1v_coefficients_device, m1v_convert_device, m1v_encode_host, m1v_encode_planes_host and m1v_convert_host
 *     return M1V_E_ARG while a plane layout is set.
 *   m1v_plane_layout_in_force(enc, &layout)   1 = a plane layout is in force (layout filled with the values the kernels use, no
 *     zeros; may be NULL), 0 = none, < 0 = error.
 * Read contract: of frame f a kernel reads only bytes of [F, F + E) rounded up to the next 4-byte boundary, where E, the frame's
 * extent, is the largest  offset + (rows - 1) * pitch + row bytes  over the three planes (rows = ye for luma, ye / 2 for chroma;
 * row bytes = xe and (xe / 2 - 1) * c_step + 1: up to the last byte the definition addresses, so that a tightly packed NV12 frame
 * has E = width * height * 3 / 2, its frame stride).  Bytes inside that range that the definition does not address (row padding, gaps
 * between planes, the surroundings of a window, chroma rows from ye / 2 on) may be read; they never influence the output. */
typedef struct m1v_plane_layout {
    size_t y_offset, cb_offset, cr_offset; /* bytes from the frame's base to sample (0,0) of each plane            */
    size_t y_pitch;                        /* bytes between luma rows; 0 = width                                   */
    size_t c_pitch;                        /* bytes between chroma rows of the addressing above; 0 = (width/2)*c_step */
    size_t c_step;                         /* bytes between neighbouring samples of ONE chroma plane: 1 or 2; 0 = 1 */
    size_t frame_stride;                   /* bytes between frames; never 0                                        */
} m1v_plane_layout;
enum { M1V_PLANES_REFERENCE = 0, M1V_PLANES_I420 = 1, M1V_PLANES_YV12 = 2, M1V_PLANES_NV12 = 3, M1V_PLANES_NV21 = 4 };
int m1v_plane_layout_preset(int width, int height, int preset, m1v_plane_layout *out);
int m1v_set_plane_layout(m1v_encoder *enc, const m1v_plane_layout *layout);
int m1v_plane_layout_in_force(const m1v_encoder *enc, m1v_plane_layout *out);

/* Sample layout: the plane layout with one more parameter, the distance between neighbouring luma samples.  It covers the YCbCr
 * frames whose samples do not lie next to one another: packed 4:2:2 (YUY2, UYVY, YVYU: capture cards, cameras, hardware JPEG
 * decoders) and P010 / P012 / P016 (10-bit and deeper hardware video decode: 16-bit little-endian words with the value in the
 * high bits, a luma plane and one plane of Cb, Cr word pairs).  For encoders created with channels = 3.
 *
 * Definition.  Frame f starts at F = d_rgb + f * frame_stride; the region coded is xe x ye as above.  The macroblock at (x, y) takes
 *     luma block k, row i, sample j       the byte at  F + y_offset + (y + 8 * (k / 2) + i) * y_pitch + (x + 8 * (k % 2) + j) * y_step
 *     chroma plane p, row i, sample j     the byte at  F + p_offset + (y / 2 + i) * c_pitch + (x / 2 + j) * c_step
 * and the record is the reference's frame body on those bytes, exactly as for plane layouts (y_step = 1 IS the plane layout).
 *
 *   m1v_sample_layout_preset(width, height, preset, &layout)   pure host arithmetic, tightly packed; y_step 2, c_step 4
 *     M1V_SAMPLES_YUY2   groups Y0 Cb Y1 Cr: y_offset 0, cb_offset 1, cr_offset 3, y_pitch 2*W, c_pitch 4*W, stride 2*W*H
 *     M1V_SAMPLES_UYVY   groups Cb Y0 Cr Y1: y_offset 1, cb_offset 0, cr_offset 2, the same pitches and stride
 *     M1V_SAMPLES_YVYU   groups Y0 Cr Y1 Cb: y_offset 0, cb_offset 3, cr_offset 1, the same pitches and stride
 *     M1V_SAMPLES_P010   y_offset 1, cb_offset 2*W*H + 1, cr_offset 2*W*H + 3, y_pitch = c_pitch = 2*W, stride 3*W*H
 *     All four need an even width and height (M1V_E_ARG otherwise); M1V_E_ARG: unknown preset.
 *     The packed 4:2:2 presets turn 4:2:2 into the 4:2:0 the format codes by taking chroma from the EVEN picture rows
 *     (c_pitch = two picture rows); a caller who wants the odd rows adds y_pitch to both chroma offsets.
 *     M1V_SAMPLES_P010 also serves P012 and P016: the bytes are the same.  The coded sample is the word's high byte, v10 >> 2 for
 *     P010: truncation, not rounding.
 *   m1v_set_sample_layout(enc, &layout)   NULL = back to the default layout.  The reconfiguration m1v_set_plane_layout is, and the
 *     same code: (y_step, c_step) = (1, 1) or (1, 2) is exactly m1v_set_plane_layout (the same kernels, the same layout in force);
 *     (2, 4) takes the tile plan behind k_encode_step2, k_size_table_step2 and k_rd_table_step2.  Everything m1v_set_plane_layout
 *     says about replacing other layouts, the calls that work on it and the packed-only entry points holds.
 *     M1V_E_ARG, before anything is launched or reallocated: a null encoder; channels != 3; a step pair other than (1, 1), (1, 2),
 *     (2, 4) (0 = 1); with c_step 4, chroma offsets more than 3 bytes apart (both components of a sample pair lie in one 4-byte
 *     group: interleaved chroma); frame_stride 0; 0 < y_pitch < width * y_step; 0 < c_pitch < (width / 2) * c_step; an offset, a
 *     pitch or a frame extent E of 2^32 or more; frame_stride < E; an encoder that a hook has forced to the run kernels.
 *   m1v_sample_layout_in_force(enc, &layout)   1 = a plane or sample layout is in force (layout filled with the values the kernels
 *     use, no zeros: y_step = 1 for a layout set through m1v_set_plane_layout; may be NULL), 0 = none, < 0 = error.  While a
 *     (2, 4) layout is in force m1v_plane_layout_in_force and m1v_input_layout return M1V_E_ARG (the message names this query).
 * Read contract: unchanged.  Of frame f a kernel reads only bytes of [F, F + E) rounded up to the next 4-byte boundary; E is
 * computed as above with luma row bytes (xe - 1) * y_step + 1 and chroma row bytes (xe / 2 - 1) * c_step + 1.  Bytes inside that
 * range that the definition does not address (the low byte of every P010 word, the chroma bytes of odd rows of a 4:2:2 frame,
 * row padding, gaps) may be read; they never influence the output. */
typedef struct m1v_sample_layout {
    size_t y_offset, cb_offset, cr_offset; /* bytes from the frame's base to sample (0,0) of each component        */
    size_t y_pitch;                        /* bytes between luma rows; 0 = width * y_step                          */
    size_t c_pitch;                        /* bytes between chroma rows of the addressing above; 0 = (width / 2) * c_step */
    size_t y_step;                         /* bytes between neighbouring luma samples: 1 or 2; 0 = 1               */
    size_t c_step;                         /* bytes between neighbouring samples of ONE chroma component: 1, 2 or 4; 0 = 1 */
    size_t frame_stride;                   /* bytes between frames; never 0                                        */
} m1v_sample_layout;
enum { M1V_SAMPLES_YUY2 = 0, M1V_SAMPLES_UYVY = 1, M1V_SAMPLES_YVYU = 2, M1V_SAMPLES_P010 = 3 };
int m1v_sample_layout_preset(int width, int height, int preset, m1v_sample_layout *out);
int m1v_set_sample_layout(m1v_encoder *enc, const m1v_sample_layout *layout);
int m1v_sample_layout_in_force(const m1v_encoder *enc, m1v_sample_layout *out);

/* RGB plane layout: frames whose R, G and B bytes lie in three planes on the device — a PyTorch image batch [n, 3, H, W] of
 * uint8, the CHW output of a JPEG decoder, three planes of a 4-plane RGBA tensor, a sliced or as_strided view of one — encoded
 * where they lie: no permute-and-copy to interleaved pixels in front of the encoder.  For encoders created with channels = 3.
 * Samples are bytes: the reference's Image::data is unsigned char.  Float samples are the float plane layout below, which writes
 * down the rounding rule the reference does not have.
 *
 * Definition.  Frame f starts at F = d_rgb + f * frame_stride.  Component c (R, G, B) of pixel (x, y) is the byte at
 *     F + c_offset + y * row_pitch + x
 * and the record of a frame is, byte for byte, the record the packed calls give for the interleaved picture [y][x] = (R, G, B) of
 * those bytes: the reference's whole frame body, colour conversion included; the same headers, first_frame_index, status bits,
 * per-frame quality and sizes.  Any byte alignment of the pointer, the offsets, the pitch and the stride is accepted.  The three
 * offsets are independent: R,G,B, B,G,R and G,B,R plane orders, three planes of a 4-plane tensor (the fourth is never read),
 * pitched windows of larger planes and planes interleaved by rows (row_pitch = 3 * width, offsets 0, width, 2 * width) are all
 * layouts.
 *
 *   m1v_rgb_plane_layout_preset(width, height, order, &layout)   pure host arithmetic (no encoder, no device): three tightly packed
 *     planes of width * height bytes, row_pitch = width, frame_stride = 3 * width * height, in memory order
 *     M1V_RGB_PLANES_RGB   R, G, B: offsets 0, W*H, 2*W*H
 *     M1V_RGB_PLANES_BGR   B, G, R: r_offset 2*W*H, g_offset W*H, b_offset 0
 *     M1V_RGB_PLANES_GBR   G, B, R: r_offset 2*W*H, g_offset 0, b_offset W*H
 *     M1V_E_ARG: a null out, width or height <= 0, an unknown order.
 *   m1v_set_rgb_plane_layout(enc, &layout)   NULL = back to the default layout.  A reconfiguration like m1v_set_input_layout (call it
 *     between batches; buffers are allocated first and swapped in on success, so a failed call leaves the encoder as it was).  The
 *     encoder takes the tile plan (m1v_path_in_use and m1v_size_table_fused are 1) behind k_encode_rgb_planes,
 *     k_size_table_rgb_planes and k_rd_table_rgb_planes.  ONE input layout is in force at a time: each of m1v_set_input_layout,
 *     m1v_set_plane_layout, m1v_set_sample_layout and m1v_set_rgb_plane_layout replaces what another has set, and each one's default
 *     (NULL; 0, 0, M1V_ORDER_RGB) restores the default plan.  While an RGB plane layout is in force m1v_input_layout,
 *     m1v_plane_layout_in_force and m1v_sample_layout_in_force return M1V_E_ARG.  Every *_device encode, probe, size-table,
 *     rd-table, budget, batch-budget and bitrate call (by size and by distortion), pipelined mode, m1v_reserve_scratch,
 *     m1v_debug_set_lds_words and m1v_delivery_* work on it.
 *     M1V_E_ARG, before anything is launched or reallocated: a null encoder; channels != 3; an odd width (the reference addresses
 *     its chroma plane with stride width / 2: with an odd width a chroma block row straddles two picture rows); row_pitch < width;
 *     (largest offset) + (height - 1) * row_pitch + width >= 2^32 (offsets inside a frame are 32-bit); two planes that share an
 *     addressed byte (their ranges may overlap as a row interleave only); frame_stride below the bytes from the smallest offset to
 *     the end of the last plane's range; an encoder that a hook has forced to the run kernels (those hooks return M1V_E_ARG on an
 *     encoder with an RGB plane layout).
 *     Packed only: m1v_coefficients_device, m1v_convert_device, m1v_encode_host, m1v_encode_planes_host and m1v_convert_host
 *     return M1V_E_ARG while an RGB plane layout is set.
 *   m1v_rgb_plane_layout_in_force(enc, &layout)   1 = an RGB plane layout is in force (layout filled with the values the kernels
 *     use; may be NULL), 0 = another layout or none, < 0 = error.
 * Read contract: of frame f a kernel reads only bytes of the three ranges [F + c_offset, F + c_offset + (height - 1) * row_pitch +
 * width), each rounded up to the next 4-byte boundary.  The kernels fetch 16-byte units: a luma unit is one strip's 16 addressed
 * bytes of one plane; a chroma unit is the 8 + 8 pixels of two neighbouring strips, and where a tile column ends with an odd strip
 * it runs 8 bytes past the half row it belongs to, in one of the first height / 4 rows of the range.  Bytes outside the three ranges
 * (a fourth plane, what lies in front of the first and behind the last frame, gaps between frames) are never read; bytes inside a
 * range that the definition does not address (row padding, another plane's rows of a row interleave) may be read and never
 * influence the output. */
typedef struct m1v_rgb_plane_layout {
    uint64_t r_offset, g_offset, b_offset; /* bytes from the frame's base to pixel (0,0) of each plane                */
    uint64_t row_pitch;                    /* bytes between picture rows, the same in the three planes; >= width      */
    uint64_t frame_stride;                 /* bytes between frames                                                    */
} m1v_rgb_plane_layout;
enum { M1V_RGB_PLANES_RGB = 0, M1V_RGB_PLANES_BGR = 1, M1V_RGB_PLANES_GBR = 2 }; /* the planes' order in memory */
int m1v_rgb_plane_layout_preset(int width, int height, int order, m1v_rgb_plane_layout *out);
int m1v_set_rgb_plane_layout(m1v_encoder *enc, const m1v_rgb_plane_layout *layout);
int m1v_rgb_plane_layout_in_force(const m1v_encoder *enc, m1v_rgb_plane_layout *out);

/* Float plane layout: frames whose R, G and B samples are floating-point numbers in three planes on the device — a PyTorch tensor
 * [n, 3, H, W] of float16, bfloat16 or float32 as a model, a colour-space stage or an augmentation pipeline produces it, three
 * planes of a 4-plane tensor, a sliced view of one — encoded where they lie: no x.mul(255).round().clamp(0, 255).to(uint8) in
 * front of the encoder.  For encoders created with channels = 3.
 *
 * Definition.  A float plane layout describes three planes of samples of one type, S bytes each: S = 2 for fp16 (IEEE binary16)
 * and bf16, S = 4 for fp32.  Frame f starts at F = d_rgb + f * frame_stride, and component c (R, G, B) of pixel (x, y) is the
 * sample at
 *     F + c_offset + y * row_pitch + x * S
 * (all quantities in bytes).  The byte of a sample is
 *     f = the sample converted to fp32                (exact for all three types)
 *     t = f * scale     one fp32 multiplication, rounded to nearest even; scale = 255.0f (M1V_RANGE_UNIT: samples 0.0 ... 1.0) or
 *                       1.0f (M1V_RANGE_BYTE: samples 0 ... 255)
 *     r = t rounded to an integer, ties to even
 *     byte = 0 if r is NaN or r < 0;  255 if r > 255;  else r
 * In numpy: np.clip(np.where(np.isnan(t), 0, np.rint(t)), 0, 255) with t = x.astype(np.float32) * np.float32(scale).  It follows
 * that -0.0, every denormal and every negative value give 0, +inf gives 255, -inf and every NaN (quiet or signalling, either
 * sign, any payload) give 0; flushing denormals cannot change a result, since every denormal, flushed or not, rounds to 0; and no
 * status bit is set for any sample value.  fp32 arithmetic because it is what a caller's own x.float() * 255 does and because
 * the product of an fp16 or bf16 sample and 255 is exact in it; ties to even because it is the default rounding of IEEE 754,
 * of torch.round and of np.rint.  The neighbours of this rule (the product rounded in fp16, the product taken in double,
 * floor(x * 255 + 0.5), ties away from zero, truncation) all differ from it on inputs that exist; tests/test_float_planes_cpu.py
 * counts them.
 * The record of a frame is then exactly what m1v_set_rgb_plane_layout gives for those bytes, which is the packed calls' record for
 * the interleaved picture [y][x] = (R, G, B): the same colour arithmetic, chroma quirk, headers, first_frame_index, per-frame
 * quality, sizes and status bits.  The three offsets are independent, as those of an RGB plane layout.
 *
 *   m1v_float_plane_layout_preset(width, height, order, sample, range, &layout)   pure host arithmetic: three tightly packed planes
 *     of width * height samples in the memory order M1V_RGB_PLANES_RGB / _BGR / _GBR, row_pitch = width * S, frame_stride = 3 *
 *     width * height * S.  M1V_E_ARG: a null out, width or height <= 0, an unknown order, sample or range.
 *   m1v_set_float_plane_layout(enc, &layout)   NULL = back to the default layout.  A reconfiguration like the other layout setters:
 *     it replaces whichever layout is in force, turns tables off, and a failed call leaves the layout and the table mode as they
 *     were.  The encoder takes the tile plan behind k_encode_float_planes, k_size_table_float_planes and k_rd_table_float_planes.
 *     While it is in force m1v_input_layout, m1v_plane_layout_in_force, m1v_sample_layout_in_force return M1V_E_ARG ("ask
 *     m1v_float_plane_layout_in_force") and m1v_rgb_plane_layout_in_force returns 0.
 *     M1V_E_ARG with a message that names the reason, before anything is launched or reallocated: a null encoder; channels != 3;
 *     an odd width; an unknown sample or range; an offset, row_pitch or frame_stride that is not a multiple of S; row_pitch <
 *     width * S; (largest offset) + (height - 1) * row_pitch + width * S >= 2^32 (offsets inside a frame are 32-bit); two planes
 *     that share bytes other than as a row interleave; frame_stride below the bytes the planes span; an encoder that a hook has
 *     forced to the run kernels.
 *     Served: every call that takes d_rgb and serves an RGB plane layout — m1v_encode_device, m1v_encode_quality_device,
 *     m1v_frame_sizes_device, m1v_frame_size_table_device, m1v_frame_rd_table_device, the budget, rd, batch-budget and bitrate
 *     encodes, pipelined mode and m1v_delivery_step.  Each returns M1V_E_ARG in front of every launch when d_rgb is not a multiple
 *     of S.  The packed-only calls refuse it as they refuse every other layout.  m1v_set_frame_table and m1v_set_plane_table
 *     return M1V_E_ARG while it is in force.
 *   m1v_float_plane_layout_in_force(enc, &layout)   1 = a float plane layout is in force (layout filled; may be NULL), 0 = another
 *     layout or none, < 0 = error.
 *   m1v_float_planes_to_bytes_device(enc, d_frames, n_frames, d_bytes, stream)   the bytes the encoder codes for these samples,
 *     by the same device function: d_bytes is uint8 [n_frames][3][height][width] in R, G, B order, tightly packed — what
 *     m1v_set_rgb_plane_layout with the M1V_RGB_PLANES_RGB preset takes.  Needs the float layout in force (M1V_E_ARG otherwise, and
 *     for null pointers, n_frames < 0 and a misaligned d_frames); asynchronous on `stream`.  A caller sees which bytes were coded;
 *     the record alone cannot show them, since most single +-1 changes of a byte leave a record unchanged.
 * Read contract: of frame f only bytes of the three ranges [F + c_offset, F + c_offset + (height - 1) * row_pitch + width * S) are
 * read, and of those only addressed samples: every load of the kernels is 8 addressed samples of one row.  Row padding, a fourth
 * plane, gaps between frames and whatever lies in front of and behind the batch are never read.
 * Not covered: float frames behind a frame table and float planes behind a plane table; float
 * YCbCr (channels-last float tensors: the float pixel layout below); value ranges other than the two named; the host-buffer entry points. */
typedef struct m1v_float_plane_layout {
    uint64_t r_offset, g_offset, b_offset; /* bytes from the frame's base to pixel (0,0) of each plane; multiples of S       */
    uint64_t row_pitch;                    /* bytes between picture rows, the same in the three planes; >= width * S         */
    uint64_t frame_stride;                 /* bytes between frames                                                           */
    int32_t sample;                        /* M1V_SAMPLE_*                                                                   */
    int32_t range;                         /* M1V_RANGE_*                                                                    */
} m1v_float_plane_layout;
enum { M1V_SAMPLE_F16 = 0, M1V_SAMPLE_BF16 = 1, M1V_SAMPLE_F32 = 2 };
enum { M1V_RANGE_UNIT = 0, M1V_RANGE_BYTE = 1 };
int m1v_float_plane_layout_preset(int width, int height, int order, int sample, int range, m1v_float_plane_layout *out);
int m1v_set_float_plane_layout(m1v_encoder *enc, const m1v_float_plane_layout *layout);
int m1v_float_plane_layout_in_force(const m1v_encoder *enc, m1v_float_plane_layout *out);
int m1v_float_planes_to_bytes_device(m1v_encoder *enc, const void *d_frames, int n_frames, uint8_t *d_bytes, void *stream);

/* Float pixel layout: frames whose R, G and B samples are floating-point numbers interleaved per pixel on the device — a PyTorch
 * tensor [n, H, W, 3] or [n, H, W, 4] of float16, bfloat16 or float32, a torch.channels_last model output (NCHW-shaped with NHWC
 * strides), a renderer's RGBA16F or RGBA32F target, a window of one — encoded where they lie: no conversion to uint8 and no
 * permute-and-copy to planes in front of the encoder.  For encoders created with channels = 3: the pixel's sample count (3 or 4)
 * is the layout's, not the encoder's.
 *
 * Definition.  Samples are of one type, S bytes each (S = 2 for fp16 and bf16, S = 4 for fp32).  d_rgb points at sample 0 of
 * pixel (0, 0) of frame 0, as for a surface.  Frame f starts at F = d_rgb + f * frame_stride, and sample i (0, 1 or 2) of pixel
 * (x, y) is the S bytes at
 *     F + y * row_pitch + x * pixel_step + i * S
 * (all quantities in bytes).  order says whether samples 0, 1, 2 are R, G, B (M1V_ORDER_RGB) or B, G, R (M1V_ORDER_BGR); with
 * pixel_step = 4 * S a 4th sample follows them and is skipped.  The byte of a sample is that of the float plane layout above
 * ("Float plane layout", Definition: f, t, r, byte), unchanged and computed by the same device function.  The record of a frame is
 * the packed calls' record for the interleaved picture [y][x] = (R, G, B) of those bytes: the same colour arithmetic, chroma quirk,
 * headers, first_frame_index, per-frame quality, sizes and status bits.
 *
 *   m1v_float_pixel_layout_preset(width, height, pixel_samples, order, sample, range, &layout)   pure host arithmetic: tightly
 *     packed pixels of pixel_samples (3 or 4) samples, pixel_step = pixel_samples * S, row_pitch = width * pixel_step,
 *     frame_stride = height * row_pitch.  M1V_E_ARG (out untouched): a null out, width or height <= 0, pixel_samples other than
 *     3 or 4, an unknown order, sample or range.
 *   m1v_set_float_pixel_layout(enc, &layout)   NULL = back to the default layout.  A reconfiguration like the other layout setters:
 *     it replaces whichever layout is in force, turns tables off, allocates first and swaps on success, and a failed call leaves
 *     the layout and the table mode as they were.  The encoder takes the tile plan behind k_float_pixels_encode,
 *     k_float_pixels_size_table and k_float_pixels_rd_table.  While it is in force m1v_input_layout, m1v_plane_layout_in_force and
 *     m1v_sample_layout_in_force return M1V_E_ARG ("ask m1v_float_pixel_layout_in_force"); m1v_rgb_plane_layout_in_force and
 *     m1v_float_plane_layout_in_force return 0.
 *     M1V_E_ARG with a message that names the reason, before anything is launched or reallocated: a null encoder; channels != 3;
 *     an odd width; an unknown order, sample or range; a pixel_step other than 3 * S or 4 * S (pixel_step == S: the message names
 *     m1v_set_float_plane_layout); a row_pitch or frame_stride that is not a multiple of S; row_pitch < width * pixel_step;
 *     (height - 1) * row_pitch + width * pixel_step >= 2^32 (offsets inside a frame are 32-bit); frame_stride below
 *     (height - 1) * row_pitch + width * pixel_step; an encoder that a hook has forced to the run kernels (those hooks return
 *     M1V_E_ARG on an encoder with this layout).
 *     Served: every call that serves the float plane layout — m1v_encode_device, m1v_encode_quality_device,
 *     m1v_frame_sizes_device, m1v_frame_size_table_device, m1v_frame_rd_table_device, the budget, rd, batch-budget and bitrate
 *     encodes by size and by distortion, pipelined mode, m1v_delivery_step with its scratch retry, the m1v_profile_* counters and
 *     m1v_debug_set_lds_words.  Each returns M1V_E_ARG in front of every launch when d_rgb is not a multiple of S.  The packed-only
 *     calls refuse it as they refuse every other layout.  m1v_set_frame_table and m1v_set_plane_table return M1V_E_ARG while it is
 *     in force.
 *   m1v_float_pixel_layout_in_force(enc, &layout)   1 = a float pixel layout is in force (layout filled; may be NULL), 0 = another
 *     layout or none, < 0 = error.
 *   m1v_float_pixels_to_bytes_device(enc, d_frames, n_frames, d_bytes, stream)   the bytes the encoder codes for these samples, by
 *     the same device function: d_bytes is uint8 [n_frames][height][width][3] in R, G, B order, tightly packed — exactly what the
 *     default packed layout encodes.  Needs this layout in force (M1V_E_ARG otherwise, and for null pointers, n_frames < 0 and a
 *     misaligned d_frames); asynchronous on `stream`.
 * Read contract: of frame f only bytes of the rows [F + y * row_pitch, F + y * row_pitch + width * pixel_step), y in 0 ...
 * height - 1, are read.  A 4th sample inside a pixel may be read and never influences the output.  Row padding, gaps between
 * frames and whatever lies in front of and behind the batch are never read (the proof, per wave, heads csrc/m1v_float_pixels.h).
 * Not covered: float pixels behind a frame table or a plane table; pixels whose colour samples do not start at sample 0 (ARGB,
 * ABGR); float YCbCr; value ranges other than the two named; the host-buffer entry points. */
typedef struct m1v_float_pixel_layout {
    uint64_t row_pitch;     /* bytes between picture rows; multiple of S; >= width * pixel_step */
    uint64_t frame_stride;  /* bytes between frames; multiple of S; >= (height - 1) * row_pitch + width * pixel_step */
    uint64_t pixel_step;    /* bytes between neighbouring pixels of a row: 3 * S or 4 * S */
    int32_t order;          /* M1V_ORDER_RGB or M1V_ORDER_BGR: samples 0, 1, 2 of a pixel; a 4th sample is skipped */
    int32_t sample;         /* M1V_SAMPLE_F16 / _BF16 / _F32 (S = 2, 2, 4) */
    int32_t range;          /* M1V_RANGE_UNIT / _BYTE */
} m1v_float_pixel_layout;
int m1v_float_pixel_layout_preset(int width, int height, int pixel_samples /* 3 or 4 */, int order, int sample, int range, m1v_float_pixel_layout *out);
int m1v_set_float_pixel_layout(m1v_encoder *enc, const m1v_float_pixel_layout *layout);   /* NULL = the default layout */
int m1v_float_pixel_layout_in_force(const m1v_encoder *enc, m1v_float_pixel_layout *out); /* 1 / 0 / < 0 */
int m1v_float_pixels_to_bytes_device(m1v_encoder *enc, const void *d_frames, int n_frames, uint8_t *d_bytes, void *stream);

/* Downscale layout: the 2:1 downscaled rendition of byte surfaces on the device — the 1080p stream beside the 4K one, a 540p proxy,
 * a thumbnail stream from a decoder pool — encoded from the full-size surfaces where they lie: no resampling kernel and no
 * full-size intermediate in front of the encoder.  width and height are the RENDITION's everywhere: the encoder is created with
 * width x height and channels = 3, and the frames it is given are 2 * width x 2 * height surfaces of 3- or 4-byte pixels (the
 * source pixel's byte count is the layout's, not the encoder's).
 *
 * Definition.  d_rgb points at byte 0 of source pixel (0, 0) of frame 0.  Frame f starts at F = d_rgb + f * frame_stride, and byte
 * i (0, 1 or 2) of source pixel (X, Y) is at
 *     F + Y * row_pitch + X * pixel_step + i
 * with pixel_step 3 or 4.  order says whether bytes 0, 1, 2 are R, G, B (M1V_ORDER_RGB) or B, G, R (M1V_ORDER_BGR); a 4th byte
 * is skipped.  The byte of colour c of rendition pixel (x, y) is
 *     (s(2x, 2y) + s(2x+1, 2y) + s(2x, 2y+1) + s(2x+1, 2y+1) + 2) >> 2
 * with s the source bytes of that colour: an exact integer that rounds half up.  The record of a frame is the packed calls' record
 * for the interleaved picture [y][x] = (R, G, B) of those bytes: the same colour arithmetic, chroma quirk, headers,
 * first_frame_index, per-frame quality, sizes and status bits.
 *
 *   m1v_downscale_layout_preset(width, height, pixel_bytes, order, factor, &layout)   pure host arithmetic: a tightly packed source,
 *     pixel_step = pixel_bytes, row_pitch = 2 * width * pixel_bytes, frame_stride = 2 * height * row_pitch.  M1V_E_ARG (out
 *     untouched): a null out, width or height <= 0, pixel_bytes other than 3 or 4, an unknown order, factor != 2.
 *   m1v_set_downscale_layout(enc, &layout)   NULL = back to the default layout.  A reconfiguration like the other layout setters:
 *     it replaces whichever layout is in force, turns tables off, allocates first and swaps on success, and a failed call leaves
 *     the layout and the table mode as they were.  The encoder takes the tile plan behind k_downscale_encode,
 *     k_downscale_size_table and k_downscale_rd_table.  While it is in force m1v_input_layout, m1v_plane_layout_in_force and
 *     m1v_sample_layout_in_force return M1V_E_ARG ("ask m1v_downscale_layout_in_force"); m1v_rgb_plane_layout_in_force,
 *     m1v_float_plane_layout_in_force and m1v_float_pixel_layout_in_force return 0.
 *     M1V_E_ARG with a message that names the reason, before anything is launched or reallocated: a null encoder; channels != 3;
 *     an odd width; an unknown order; factor != 2; a pixel_step other than 3 or 4; row_pitch < 2 * width * pixel_step;
 *     (2 * height - 1) * row_pitch + 2 * width * pixel_step >= 2^32 (offsets inside a frame are 32-bit); frame_stride below
 *     (2 * height - 1) * row_pitch + 2 * width * pixel_step; an encoder that a hook has forced to the run kernels (those hooks
 *     return M1V_E_ARG on an encoder with this layout).  Any byte alignment of d_rgb, row_pitch and frame_stride is accepted, as
 *     for a surface: a window may start at any pixel of a larger surface.
 *     Served: every call that serves the float pixel layout — m1v_encode_device, m1v_encode_quality_device,
 *     m1v_frame_sizes_device, m1v_frame_size_table_device, m1v_frame_rd_table_device, the budget, rd, batch-budget, bitrate,
 *     streams and streams-budget encodes, pipelined mode, m1v_delivery_step with its scratch retry, the m1v_profile_* counters and
 *     m1v_debug_set_lds_words.  The packed-only calls refuse it as they refuse every other layout.  m1v_set_frame_table and
 *     m1v_set_plane_table return M1V_E_ARG while it is in force.
 *   m1v_downscale_layout_in_force(enc, &layout)   1 = a downscale layout is in force (layout filled; may be NULL), 0 = another
 *     layout or none, < 0 = error.
 *   m1v_downscale_to_bytes_device(enc, d_frames, n_frames, d_bytes, stream)   the bytes the encoder codes for these surfaces:
 *     d_bytes is uint8 [n_frames][height][width][3] in R, G, B order, tightly packed — exactly what the default packed layout
 *     encodes.  Needs this layout in force (M1V_E_ARG otherwise, and for null pointers and n_frames < 0); asynchronous on `stream`.
 * Read contract: of frame f only bytes of the source rows [F + Y * row_pitch, F + Y * row_pitch + 2 * width * pixel_step), Y in
 * 0 ... 2 * height - 1, are read.  A 4th byte inside a pixel may be read and never influences the output.  Row padding, gaps
 * between frames and whatever lies around the batch are never read (the proof, per wave, heads csrc/m1v_downscale.h).
 * Not covered: factor 4 and other factors (the field exists so that they can follow); filters other than the box; sources of odd
 * extent; downscaled YCbCr planes, RGB planes and float layouts; the layout behind a frame table or a plane table; the host-buffer
 * entry points and the folder CLI; several renditions in one pass. */
typedef struct m1v_downscale_layout {
    uint64_t row_pitch;     /* bytes between SOURCE rows; >= 2 * width * pixel_step */
    uint64_t frame_stride;  /* bytes between source frames; >= (2 * height - 1) * row_pitch + 2 * width * pixel_step */
    uint64_t pixel_step;    /* bytes between neighbouring source pixels of a row: 3 or 4 */
    int32_t order;          /* M1V_ORDER_RGB or M1V_ORDER_BGR: bytes 0, 1, 2 of a source pixel; a 4th byte is skipped */
    int32_t factor;         /* 2; anything else is M1V_E_ARG */
} m1v_downscale_layout;     /* 32 bytes, offsets 0, 8, 16, 24, 28 */
int m1v_downscale_layout_preset(int width, int height, int pixel_bytes /* 3 or 4 */, int order, int factor, m1v_downscale_layout *out);
int m1v_set_downscale_layout(m1v_encoder *enc, const m1v_downscale_layout *layout);   /* NULL = the default layout */
int m1v_downscale_layout_in_force(const m1v_encoder *enc, m1v_downscale_layout *out); /* 1 / 0 / < 0 */
int m1v_downscale_to_bytes_device(m1v_encoder *enc, const void *d_frames, int n_frames, uint8_t *d_bytes, void *stream);

/* Downscale plane layout: the 2:1 downscaled rendition of planar and semi-planar YCbCr frames on the device — the 1080p stream of
 * a decoder pool's 4K NV12 surfaces, the proxy of a camera's I420 frames — encoded from the full-size planes where they lie: no
 * resampling kernel and no intermediate in front of the encoder, and no detour through RGB.  width and height are the
 * RENDITION's everywhere: the encoder is created with width x height and channels = 3, and the frames it is given are true 4:2:0
 * sources of 2 * width x 2 * height luma samples and width x height samples per chroma component.
 *
 * Definition.  Source addressing is the plane layout's: frame f starts at F = d_rgb + f * frame_stride,
 *     source luma sample (X, Y) is at                F + y_offset + Y * y_pitch + X
 *     source sample (U, V) of chroma plane p is at   F + p_offset + V * c_pitch + U * c_step
 * with c_step 1 (one plane per component: I420, YV12) or 2 (interleaved pairs: NV12, NV21).  The rendition's luma sample (x, y) is
 *     (s(2x, 2y) + s(2x+1, 2y) + s(2x, 2y+1) + s(2x+1, 2y+1) + 2) >> 2
 * with s the source luma samples, and sample (u, v) of chroma plane p, u < width / 2, v < height / 2, is the same expression over
 * that plane's source samples (2u, 2v) ... (2u+1, 2v+1): an exact integer that rounds half up.  This is a box filter per plane,
 * with no chroma-siting correction.  The record of a frame is, byte for byte, the record the plane layout (m1v_set_plane_layout)
 * gives for the tightly packed M1V_PLANES_I420 frame of those rendition samples: the same headers, first_frame_index, status bits,
 * per-frame quality and sizes.  (The plane formula on a true 4:2:0 plane is ordinary 4:2:0 sampling: the reference's chroma quirk
 * plays no part.)  The reference-style 4:4:4 planes (M1V_PLANES_REFERENCE) are not a source of this kind.
 *
 *   m1v_downscale_plane_layout_preset(width, height, preset, factor, &layout)   pure host arithmetic: the tightly packed
 *     2 * width x 2 * height source of M1V_PLANES_I420, _YV12, _NV12 or _NV21; width and height are the rendition's.  M1V_E_ARG
 *     (out untouched): a null out, M1V_PLANES_REFERENCE, an unknown preset, an odd or non-positive width or height, factor != 2.
 *   m1v_set_downscale_plane_layout(enc, &layout)   NULL = back to the default layout.  A reconfiguration like the other layout
 *     setters: it replaces whichever layout is in force, turns tables off, allocates first and swaps on success, and a failed call
 *     leaves the layout and the table mode as they were.  The encoder takes the tile plan behind k_half_planes_encode,
 *     k_half_planes_size_table and k_half_planes_rd_table.  While it is in force m1v_input_layout, m1v_plane_layout_in_force and
 *     m1v_sample_layout_in_force return M1V_E_ARG ("ask m1v_downscale_plane_layout_in_force"); the getters of the other kinds
 *     return 0.
 *     M1V_E_ARG with a message that names the reason, before anything is launched or reallocated: a null encoder; channels != 3;
 *     an odd width or height; factor != 2; reserved != 0; c_step > 2; frame_stride == 0; 0 < y_pitch < 2 * width;
 *     0 < c_pitch < width * c_step; a source extent E of 2^32 or more (offsets inside a frame are 32-bit); frame_stride < E; an
 *     encoder that a hook has forced to the run kernels (those hooks return M1V_E_ARG on an encoder with this layout).
 *     E is the plane layout's extent taken on the source: the largest offset + (rows - 1) * pitch + row bytes over the three
 *     planes, with rows = 2 * ye for luma and ye for chroma, row bytes = 2 * xe for luma and (xe - 1) * c_step + 1 for chroma, and
 *     xe x ye the coded region in rendition samples (16 * m1v_strips x 16 * m1v_mb_rows).  Any byte alignment of d_rgb, offsets,
 *     pitches and stride is accepted.  Planes with c_step = 2 that are not interleaved with each other work too.
 *     Served: every call that serves the downscale layout — m1v_encode_device, m1v_encode_quality_device,
 *     m1v_frame_sizes_device, m1v_frame_size_table_device, m1v_frame_rd_table_device, the budget, rd, batch-budget, bitrate,
 *     streams and streams-budget encodes, pipelined mode, m1v_delivery_step with its scratch retry, the m1v_profile_* counters and
 *     m1v_debug_set_lds_words.  The packed-only calls refuse it as they refuse every other layout.  m1v_set_frame_table and
 *     m1v_set_plane_table return M1V_E_ARG while it is in force.
 *   m1v_downscale_plane_layout_in_force(enc, &layout)   1 = a downscale plane layout is in force (layout filled with the values the
 *     kernels use, no zeros; may be NULL), 0 = another layout or none, < 0 = error.
 *   m1v_downscale_planes_to_i420_device(enc, d_src, n_frames, d_dst, stream)   the samples the encoder codes for these frames:
 *     d_dst is uint8 [n_frames][width * height * 3 / 2], tightly packed I420 whatever the source's form — exactly what
 *     m1v_set_plane_layout with the M1V_PLANES_I420 preset encodes.  An elementwise kernel over the whole width x height rendition
 *     (every addressed byte of the 2 * width x 2 * height source is read, and addressed bytes only): the reference for the bytes,
 *     not a fast path.  Needs this layout in force (M1V_E_ARG otherwise, and for null pointers and n_frames < 0).  Because it
 *     reads the whole source and the setter holds a layout only to the coded region's extent E, it also returns M1V_E_ARG when
 *     the extent of the whole source (E with xe x ye = width x height) is 2^32 or more or exceeds frame_stride: an encoder in
 *     strict mode, or of a width or height that is no multiple of 16.  Asynchronous on `stream`.
 * Read contract: of frame f only bytes of [F, F + E) rounded up to the next 4-byte boundary are read by the encoding calls (the
 * boundary is counted from F, whatever F's own alignment).
 * Unaddressed bytes inside that range (row padding, gaps between planes, the other component's bytes of a c_step = 2 plane) may
 * be read and never influence the output.  Gaps between frames and whatever lies around the batch are never read (the proof, per
 * wave, heads csrc/m1v_downscale_planes.h).
 * Not covered: factor 4 and other filters (the factor field exists so that they can follow); sources of odd extent; 4:4:4 and
 * reference-style planes; 4:2:2 and P010 sources; RGB-plane and float sources; the kind behind a frame table or a plane table;
 * the host-buffer entry points and the folder CLI; several renditions in one pass. */
typedef struct m1v_downscale_plane_layout {
    uint64_t y_offset, cb_offset, cr_offset;  /* of the SOURCE, bytes from the frame's base                 */
    uint64_t y_pitch;                         /* 0 = 2 * width                                              */
    uint64_t c_pitch;                         /* 0 = width * c_step                                         */
    uint64_t c_step;                          /* 1 or 2; 0 = 1                                              */
    uint64_t frame_stride;                    /* never 0                                                    */
    int32_t  factor;                          /* 2                                                          */
    int32_t  reserved;                        /* 0                                                          */
} m1v_downscale_plane_layout;                 /* 64 bytes */
int m1v_downscale_plane_layout_preset(int width, int height, int preset, int factor, m1v_downscale_plane_layout *out);
int m1v_set_downscale_plane_layout(m1v_encoder *enc, const m1v_downscale_plane_layout *layout);  /* NULL = default layout */
int m1v_downscale_plane_layout_in_force(const m1v_encoder *enc, m1v_downscale_plane_layout *out); /* 1 / 0 / < 0 */
int m1v_downscale_planes_to_i420_device(m1v_encoder *enc, const void *d_src, int n_frames, void *d_dst, void *stream);

/* Downscale word layout: the 2:1 downscaled rendition of YCbCr frames with 16-bit samples on the device — the 1080p stream of a
 * decoder's 4K 10-bit material, handed out as P010 (P012, P016) by a hardware decoder or as yuv420p10le / yuv420p12le by a
 * software decoder — encoded from the full-size planes where they lie: no resampling kernel and no intermediate in front of the
 * encoder, and the average is taken on the words, before any bit is dropped.  width and height are the RENDITION's everywhere:
 * the encoder is created with width x height and channels = 3, and the frames it is given are true 4:2:0 sources of
 * 2 * width x 2 * height luma words and width x height words per chroma component.  Every sample is a 16-bit little-endian word.
 *
 * Definition.  Frame f starts at F = d_rgb + f * frame_stride,
 *     source luma word (X, Y) is at                  F + y_offset + Y * y_pitch + 2 * X
 *     source word (U, V) of chroma plane p is at     F + p_offset + V * c_pitch + U * c_step
 * with c_step 2 (one plane per component: yuv420p10le and its kin) or 4 (interleaved Cb, Cr word pairs: P010; as in
 * m1v_set_sample_layout the two chroma offsets are then at most 3 bytes apart).  A rendition sample is computed in two steps over
 * its own plane's source words w, for luma sample (x, y) and likewise for sample (u, v) of chroma plane p, u < width / 2,
 * v < height / 2:
 *     a = (w(2x, 2y) + w(2x+1, 2y) + w(2x, 2y+1) + w(2x+1, 2y+1) + 2) >> 2
 *     sample = min(a >> shift, 255)
 * a is an exact integer that rounds half up, taken at the full word precision; the >> shift truncates, as the sample layout's
 * P010 rule does.  shift is 0 .. 8: 8 for high-aligned words (P010 / P012 / P016, yuv420p16le), 2 for low-aligned 10-bit words, 4
 * for low-aligned 12-bit words.  The min defines what bits above the stated depth do.  This is a box filter per plane,
 * with no chroma-siting correction.  The record of a frame is, byte for byte, the record the plane layout (m1v_set_plane_layout)
 * gives for the tightly packed M1V_PLANES_I420 frame of those rendition samples: the same headers, first_frame_index, status
 * bits, per-frame quality and sizes.
 *
 *   m1v_downscale_word_layout_preset(width, height, preset, factor, &layout)   pure host arithmetic: the tightly packed
 *     2 * width x 2 * height source; width and height are the rendition's, W and H below.
 *         preset                               shift  c_step  y_pitch  c_pitch  cb_offset  cr_offset  frame_stride
 *         M1V_WORDS_P010 (also P012 and P016)  8      4       4W       4W       8WH        8WH + 2    12WH
 *         M1V_WORDS_I010                       2      2       4W       2W       8WH        10WH       12WH
 *         M1V_WORDS_I012                       4      2       4W       2W       8WH        10WH       12WH
 *         M1V_WORDS_I016                       8      2       4W       2W       8WH        10WH       12WH
 *     M1V_E_ARG (out untouched): a null out, an unknown preset, an odd or non-positive width or height, factor != 2.
 *   m1v_set_downscale_word_layout(enc, &layout)   NULL = back to the default layout.  A reconfiguration like the other layout
 *     setters: it replaces whichever layout is in force, turns tables off, allocates first and swaps on success, and a failed call
 *     leaves the layout and the table mode as they were.  The encoder takes the tile plan behind k_half_words_encode,
 *     k_half_words_size_table and k_half_words_rd_table.  While it is in force m1v_input_layout, m1v_plane_layout_in_force and
 *     m1v_sample_layout_in_force return M1V_E_ARG ("ask m1v_downscale_word_layout_in_force"); the getters of the other kinds
 *     return 0.
 *     M1V_E_ARG with a message that names the reason, before anything is launched or reallocated: a null encoder; channels != 3;
 *     an odd width or height; factor != 2; shift outside 0 .. 8; c_step other than 2 or 4 (0 = 2); with c_step 4, chroma offsets
 *     more than 3 bytes apart; frame_stride == 0; 0 < y_pitch < 4 * width; 0 < c_pitch < width * c_step; a source extent E of
 *     2^32 or more (offsets inside a frame are 32-bit); frame_stride < E; an encoder that a hook has forced to the run kernels
 *     (those hooks return M1V_E_ARG on an encoder with this layout).
 *     E is the plane layout's extent taken on the source: the largest offset + (rows - 1) * pitch + row bytes over the three
 *     planes, with rows = 2 * ye for luma and ye for chroma, row bytes = 4 * xe for luma and (xe - 1) * c_step + 2 for chroma, and
 *     xe x ye the coded region in rendition samples (16 * m1v_strips x 16 * m1v_mb_rows).  Any byte alignment of d_rgb, offsets,
 *     pitches and stride is accepted.
 *     Served: every call that serves the downscale plane layout — m1v_encode_device, m1v_encode_quality_device,
 *     m1v_frame_sizes_device, m1v_frame_size_table_device, m1v_frame_rd_table_device, the budget, rd, batch-budget, bitrate,
 *     streams and streams-budget encodes, pipelined mode, m1v_delivery_step with its scratch retry, the m1v_profile_* counters and
 *     m1v_debug_set_lds_words.  The packed-only calls refuse it as they refuse every other layout.  m1v_set_frame_table and
 *     m1v_set_plane_table return M1V_E_ARG while it is in force.
 *   m1v_downscale_word_layout_in_force(enc, &layout)   1 = a downscale word layout is in force (layout filled with the values the
 *     kernels use, no zeros but a shift of 0; may be NULL), 0 = another layout or none, < 0 = error.
 *   m1v_downscale_words_to_i420_device(enc, d_src, n_frames, d_dst, stream)   the samples the encoder codes for these frames:
 *     d_dst is uint8 [n_frames][width * height * 3 / 2], tightly packed I420 whatever the source's form — exactly what
 *     m1v_set_plane_layout with the M1V_PLANES_I420 preset encodes.  An elementwise kernel over the whole width x height rendition
 *     (every addressed byte of the 2 * width x 2 * height source is read, and addressed bytes only): the reference for the bytes,
 *     not a fast path.  Needs this layout in force (M1V_E_ARG otherwise, and for null pointers and n_frames < 0).  Because it
 *     reads the whole source and the setter holds a layout only to the coded region's extent E, it also returns M1V_E_ARG when
 *     the extent of the whole source (E with xe x ye = width x height) is 2^32 or more or exceeds frame_stride: an encoder in
 *     strict mode, or of a width or height that is no multiple of 16.  Asynchronous on `stream`.
 * Read contract: of frame f only bytes of [F, F + E) rounded up to the next 4-byte boundary are read by the encoding calls (the
 * boundary is counted from F, whatever F's own alignment).
 * Unaddressed bytes inside that range (row padding, gaps between planes, the other component's words of a c_step = 4 plane) may
 * be read and never influence the output.  Gaps between frames and whatever lies around the batch are never read (the proof, per
 * wave, heads csrc/m1v_downscale_words.h).
 * Not covered: factor 4 and other filters (the factor field exists so that they can follow); sources of odd extent; big-endian
 * words; 4:2:2 and 4:4:4 word sources (P210, Y210, yuv422p10le); rounding instead of truncation at the shift; the kind behind a
 * frame table or a plane table; the host-buffer entry points and the folder CLI; several renditions in one pass. */
typedef struct m1v_downscale_word_layout {
    uint64_t y_offset, cb_offset, cr_offset;  /* of the SOURCE, bytes from the frame's base                 */
    uint64_t y_pitch;                         /* bytes between source luma rows; 0 = 4 * width              */
    uint64_t c_pitch;                         /* bytes between source chroma rows; 0 = width * c_step       */
    uint64_t c_step;                          /* 2 or 4; 0 = 2                                              */
    uint64_t frame_stride;                    /* never 0                                                    */
    int32_t  factor;                          /* 2                                                          */
    int32_t  shift;                           /* 0 .. 8                                                     */
} m1v_downscale_word_layout;                  /* 64 bytes, offsets 0, 8, ... 48, 56, 60 */
enum { M1V_WORDS_P010 = 0, M1V_WORDS_I010 = 1, M1V_WORDS_I012 = 2, M1V_WORDS_I016 = 3 };
int m1v_downscale_word_layout_preset(int width, int height, int preset, int factor, m1v_downscale_word_layout *out);
int m1v_set_downscale_word_layout(m1v_encoder *enc, const m1v_downscale_word_layout *layout);  /* NULL = default layout */
int m1v_downscale_word_layout_in_force(const m1v_encoder *enc, m1v_downscale_word_layout *out); /* 1 / 0 / < 0 */
int m1v_downscale_words_to_i420_device(m1v_encoder *enc, const void *d_src, int n_frames, void *d_dst, void *stream);

/* Frame table: a batch whose frames lie at separate device addresses — the surfaces of a decoder's pool in the order the pool
 * recycles them, a capture ring, a list of tensors, frames 5, 2, 9 of a larger buffer — encoded where they lie: no gather into a
 * contiguous batch in front of the encoder.
 *
 * Definition.  While the table is on, the d_rgb argument of every *_device call and of m1v_delivery_step is a device array of
 * uint64_t[n_frames] that holds the device address of each frame's base F; it is no longer the first frame's first byte, and frame
 * f no longer starts at d_rgb + f * frame_stride.  Everything else the layout in force defines — offsets, pitches, steps, byte
 * order, the read contract — applies to each F exactly as it does without a table.  Frame f of the table is frame
 * first_frame_index + f of the stream.  Entries may repeat an address, appear in any memory order and point into different
 * allocations; any byte alignment of an entry is accepted, as any pointer, pitch and stride are without a table.
 *
 *   m1v_set_frame_table(enc, enable)   M1V_OK, or M1V_E_ARG: a null encoder; enable != 0 on the default packed layout.  The table
 *     needs a layout served by the tile kernels in force (m1v_set_input_layout, m1v_set_plane_layout, m1v_set_sample_layout,
 *     m1v_set_rgb_plane_layout; not m1v_set_float_plane_layout, which takes no table); packed frames go through a table after m1v_set_input_layout(enc, width * channels, 0, order), the
 *     way a packed buffer reaches the surface kernels.  The packed tile kernels and the run kernels take no table.
 *     The flag is part of the layout in force: every successful layout setter, those that restore the default included, turns it
 *     off; a setter that fails leaves it as it was, like everything else.  Not a reconfiguration: nothing is allocated, waited for
 *     or queued, and the plan does not change.  m1v_path_in_use, m1v_size_table_fused and the layout getters answer as before; the
 *     layout's frame_stride is kept and reported, and unused while the table is on.
 *   m1v_frame_table(enc)   1 = on, 0 = off, -1 = a null encoder.
 * Served: m1v_encode_device, m1v_encode_quality_device, m1v_frame_sizes_device, m1v_frame_size_table_device,
 * m1v_frame_rd_table_device, the budget, batch-budget and bitrate calls by size and by distortion, pipelined mode, and
 * m1v_delivery_step with its scratch retry, which reads the table again.
 * When the table is read: only the kernels read it, on the stream, and only entries [0, n_frames).  A caller may fill it with work
 * queued on the same stream in front of the call, with no host wait.  The table and the frames it names must stay valid as long
 * as d_rgb must without a table; for a delivery step that is until the batch's copy has started.
 * Errors: M1V_E_ARG before anything is launched when the table pointer is not 8-byte aligned (the kernels load an entry as one
 * 64-bit word); the null and n_frames checks are those of every call.  The entries are not validated and cannot be: an entry that
 * is not a device address of the encoder's device is undefined behaviour, exactly as a bad d_rgb is without a table.
 * Read contract: unchanged per frame — the range or ranges the layout defines, relative to that frame's F, each rounded up to the
 * next 4-byte boundary; of the table, entries [0, n_frames).
 * Separate pointers per plane of one frame (Y, Cb and Cr, or R, G and B, in three allocations) are the plane table below.
 * Not covered by either table: P010 planes behind separate Y and UV pointers (a (2, 4) sample layout takes a frame table only),
 * float frames and float planes (m1v_set_float_plane_layout: both setters return M1V_E_ARG while it is in force), and
 * the host-buffer entry points (m1v_encode_host, m1v_encode_planes_host), which take no table. */
int m1v_set_frame_table(m1v_encoder *enc, int enable);
int m1v_frame_table(const m1v_encoder *enc);

/* Plane table: a batch whose frames' planes lie at separate device addresses — AVFrame::data[0..2] with linesize[], the Y pointer
 * and the UV pointer of a decoder's NV12 surface, three separately allocated tensors of a colour-space stage, the r, g, b =
 * x.unbind(1) planes of tensors that were never one allocation — encoded where they lie: no copy of the planes into one frame.
 *
 * Definition.  While the plane table is on, the d_rgb argument of every *_device call and of m1v_delivery_step is a device array of
 * uint64_t[n_frames][3]: entry [f][p] is the device address P of plane p of frame f, in the order Y, Cb, Cr under a plane layout
 * and R, G, B under an RGB plane layout.  The layout in force applies to each plane relative to its own pointer: sample (0, 0) of
 * plane p lies at P + p_offset, and the pitches, c_step, the chroma quirk, the record, its headers, first_frame_index, the status
 * bits and per-frame quality are exactly those without a table.  NV12 and NV21 need no format of their own: [f][1] and [f][2] both
 * hold the UV plane's pointer under chroma offsets 0 and 1 (1 and 0), or [f][2] = [f][1] + 1 under offsets 0 and 0.  Entries may
 * repeat, alias, come in any memory order and point into different allocations; any byte alignment of an entry is accepted.  The
 * layout's frame_stride is kept and reported, and unused, as with a frame table.
 *
 *   m1v_set_plane_table(enc, enable)   M1V_OK, or M1V_E_ARG with a message that names the reason: a null encoder; enable != 0 on
 *     the packed layout (no planes), on a surface layout (one plane: a frame table serves it), or on a (2, 4) sample layout (packed
 *     4:2:2 has no planes; P010 behind separate Y and UV pointers is not covered).  Served layouts: m1v_set_plane_layout, which is
 *     the sample steps (1, 1) and (1, 2), and m1v_set_rgb_plane_layout.
 *     The table mode is one field of the layout in force: off, frames or planes.  m1v_set_frame_table and m1v_set_plane_table with
 *     enable != 0 each select their own mode, replacing the other; either of them with 0 turns tables off.  Every successful layout
 *     setter turns tables off; a setter that fails leaves the mode as it was.  Not a reconfiguration: nothing is allocated, waited
 *     for or queued, and the plan does not change.
 *   m1v_plane_table(enc)   1 = the plane table is on, 0 = off or a frame table, -1 = a null encoder.  (m1v_frame_table answers 1 in
 *     frame mode only.)
 * Served: every call a frame table serves, m1v_delivery_step's scratch retry included, which passes the pointer on again.
 * When the table is read: only the kernels read it, on the stream, and only entries [0, n_frames)[0, 3).  A caller may fill it
 * with work queued on the same stream directly in front of the call.  The host's one check is that d_rgb is 8-byte aligned:
 * M1V_E_ARG in front of every launch otherwise.  The entries are not validated, as a frame table's are not.
 * Read contract, per plane.  Of plane p of frame f only bytes of [P, P + E_p), rounded up to the next 4-byte boundary, are read:
 *     E_p = p_offset + (rows_p - 1) * pitch_p + row_bytes_p
 * with the rows and row bytes of the contracts above: ye rows of xe bytes for Y, ye / 2 rows of (xe / 2 - 1) * c_step + 1 bytes for
 * Cb and Cr (xe, ye = the coded region); for an RGB plane layout the layout's own range per plane, relative to P: [P + c_offset,
 * P + c_offset + (height - 1) * row_pitch + width).  No byte outside the three ranges is read, and bytes inside a range that the
 * definition does not address never influence the output.  Each chroma plane is held to its own range: where the single-base
 * kernels move a 16-byte unit back at the end of the frame's extent, these move it back at the end of its own plane's (a 16 x 16
 * I420 picture has chroma planes of 64 bytes, and the last unit of each still starts and ends inside them).  With [f][2] =
 * [f][1] + 1 the rounding is relative to that pointer: the Cr range of a tightly packed NV12 plane then ends one byte behind the
 * plane, which the two-offset form avoids.
 * Not covered: P010 planes; float planes (m1v_set_float_plane_layout); the host-buffer entry points. */
int m1v_set_plane_table(m1v_encoder *enc, int enable);
int m1v_plane_table(const m1v_encoder *enc);

/* An encoder is driven from ONE stream.  Every call adds into one of two internal counter sets, and the assembly kernel of
 * call k clears the set that call k + 1 adds into; calls on different streams would race on them.  After an error return
 * the failed call's outputs are undefined, and the next call on the same encoder and stream is exact again.
 *
 * Pipelined mode (off by default).  When on, m1v_encode_device launches only the encode kernel on `stream`;
 * the run layout (run kernels) and the assembly into d_out (k_assemble) run on an internal stream, so the NEXT
 * batch's encode kernel (launched on `stream`) overlaps them.  d_out / d_frame_sizes / d_total / d_status of a batch
 * are complete once work enqueued behind m1v_flush(enc, s) on stream s has started; callers double-buffer d_out.  The
 * internal scratch is double-buffered, so at most two batches are in flight. */
int m1v_set_pipelined(m1v_encoder *enc, int enable);
/* Makes `stream` wait for every gather still pending on the internal stream.  An encoder in pipelined mode is meant to
 * be driven from ONE stream; calls on another stream are still ordered behind the gather that last used their set
 * of internal buffers. */
int m1v_flush(m1v_encoder *enc, void *stream);

/* Overlapped delivery of the frame records to the HOST (the path ends in a host bitstream: the reference writes it with
 * bitvector_fwrite, include/encoder.h:445).  Input resident in device memory; the device-to-host copy of batch k runs on an
 * internal stream under the encode of batch k+1, through two device output buffers and two pinned host buffers owned by the
 * delivery object.  Nothing is allocated inside the loop; one host wait per step (for 16 bytes: the batch's byte count and
 * status word).  A batch that ran out of overflow scratch is encoded again with the worst case reserved; any other status
 * bit fails the step (nothing of an undefined batch is delivered).
 *
 *   m1v_delivery_create(enc, out_cap, &d)      out_cap = capacity of each output buffer in bytes (0: max_frames x frame bound)
 *   slot = m1v_delivery_step(d, d_rgb, n, first_index, stream)
 *                                              queues the encode of this batch on `stream`, then starts the copy of the batch
 *                                              BEFORE it; returns that batch's slot (0 or 1), M1V_DELIVERY_NONE on the first
 *                                              call, or a negative M1V_E_*.  d_rgb must stay valid until the batch's copy has started.
 *   slot = m1v_delivery_flush(d)               starts the copy of the last batch (M1V_DELIVERY_NONE if none is pending)
 *   m1v_delivery_wait(d, slot, &host, &bytes, &frame_sizes)
 *                                              blocks until that slot's copy has arrived; host / frame_sizes point into the
 *                                              slot's pinned buffers, valid until the second step after the one that returned it
 * The delivery object must not be stepped or flushed after its encoder has been destroyed (wait and destroy are fine). */
typedef struct m1v_delivery m1v_delivery;
enum { M1V_DELIVERY_NONE = 2 };
int m1v_delivery_create(m1v_encoder *enc, size_t out_cap, m1v_delivery **out);
void m1v_delivery_destroy(m1v_delivery *d);
int m1v_delivery_step(m1v_delivery *d, const uint8_t *d_rgb, int n_frames, int first_frame_index, void *stream);
int m1v_delivery_flush(m1v_delivery *d);
int m1v_delivery_wait(m1v_delivery *d, int slot, const uint8_t **host, uint64_t *bytes, const uint64_t **frame_sizes);
uint64_t m1v_delivery_bytes(const m1v_delivery *d, int slot); /* bytes of the batch in `slot`: known once its copy has been started */

/* Device memory for callers that do not link the HIP runtime themselves (a plain-C caller of m1v_encode_device /
 * m1v_delivery_step, tests/delivery_main.c): hipMalloc / hipFree on the current device.  NULL on failure. */
void *m1v_alloc_device(size_t bytes);
void m1v_free_device(void *p);

/* Starts the GPU runtime for `device` (context, code objects) so that a later m1v_create() does not pay for it.
 * Optional; meant to be called from another thread while the caller is still busy with host work. */
int m1v_warm_up(int device);

/* Host-buffer convenience (PCIe inclusive, synchronous): returns total bytes or negative M1V_E_*. */
long m1v_encode_host(m1v_encoder *enc, const uint8_t *rgb, int n_frames, int first_frame_index,
                     uint8_t *out, size_t out_cap, uint64_t *frame_sizes);

/* m1v_encode_host plus, when planes != NULL, the full-resolution Y/Cb/Cr planes of m1v_convert_host from the SAME
 * upload (what one frame-loop iteration of the reference produces: its frame record, encoder.h:196-458, and the
 * content of image_<k>.bit, encoder.h:461-465).  The upload runs in two halves so the download of the first
 * half's planes (PCIe is full duplex) overlaps the upload of the second. */
long m1v_encode_planes_host(m1v_encoder *enc, const uint8_t *rgb, int n_frames, int first_frame_index,
                            uint8_t *out, size_t out_cap, uint64_t *frame_sizes, uint8_t *planes);

/* Pinned host memory for the buffers handed to the *_host entry points (optional; any host pointer works, pinned
 * ones are copied at the PCIe rate). */
void *m1v_alloc_host(size_t bytes);
void m1v_free_host(void *p);

/* The 64 zigzag-ordered quantised levels of every visited block, int16, in emission order
 * [frame][strip][macroblock][Y0 Y1 Y2 Y3 Cb Cr][64].  Packed input only (as m1v_convert_* and the *_host entry points):
 * M1V_E_ARG while a surface layout is set. */
int m1v_coefficients_device(m1v_encoder *enc, const uint8_t *d_rgb, int n_frames, int16_t *d_coeffs,
                            void *stream);

/* Full-resolution planes per frame: Y[w*h] Cb[w*h] Cr[w*h] (3*w*h bytes per frame). */
int m1v_convert_device(m1v_encoder *enc, const uint8_t *d_rgb, int n_frames, uint8_t *d_planes,
                       void *stream);
/* Host-buffer form of m1v_convert_device (synchronous; feeds the image_<k>.bit side files). */
int m1v_convert_host(m1v_encoder *enc, const uint8_t *rgb, int n_frames, uint8_t *planes);
/* 2x2 truncated mean of one Cb and one Cr plane (even width and height). */
int m1v_subsample_device(m1v_encoder *enc, const uint8_t *d_cb, const uint8_t *d_cr,
                         uint8_t *d_cb_sub, uint8_t *d_cr_sub, void *stream);

/* byte k of frame f = byte (k & 7) of splitmix64(seed + f*0x9E3779B97F4A7C15 + (k >> 3)), little-endian */
int m1v_synth_device(uint8_t *d_rgb, size_t bytes_per_frame, int n_frames, uint64_t seed,
                     uint64_t first_frame_index, void *stream);

/* Kernel timing by HIP events recorded on the launch stream around the dominant kernel
 * (k_encode_tiles; k_encode_dense / k_encode_strips on the run path; k_size_table_tiles / k_size_table_rgba for a size-table pass,
 * the k_rd_table_* kernels for an rd-table pass;
 * k_encode_surface / k_size_table_surface on a surface layout).  enable!=0 starts collecting; m1v_profile_read synchronises the recorded events
 * and returns launches/total milliseconds since the last read. */
int m1v_profile_enable(m1v_encoder *enc, int enable);
int m1v_profile_read(m1v_encoder *enc, int *launches, double *total_ms);
/* The same, one duration per launch: ms[0 .. min(cap, *launches)) in launch order (for min / median / spread). */
int m1v_profile_read_times(m1v_encoder *enc, float *ms, int cap, int *launches);

/* Test hook: capacity in 32-bit words of the per-strip LDS bit buffer (0 = default).  A tiny value
 * forces the global-memory fallback path so that tests can cover it. */
int m1v_debug_set_lds_words(m1v_encoder *enc, int words);
/* Two encode kernels serve the path.  TILES (default for 3-channel pictures of any width and alignment): a workgroup
 * owns 8 adjacent strips x 4 macroblock rows and brings the pixels in as whole 128-byte lines by LDS-DMA.  RUNS (4-channel
 * pictures): a workgroup owns 256 consecutive blocks of the stream, every lane loads its own 24-byte block rows.  Both
 * produce the same bytes.  Test hook: -1 = by geometry, 0 = runs, 1 = tiles (3 channels only).  (A surface layout,
 * m1v_set_input_layout, runs the tile workgroup for 3 and 4 channels and reports 1.) */
int m1v_debug_set_path(m1v_encoder *enc, int path);
int m1v_path_in_use(const m1v_encoder *enc); /* 1 = tiles, 0 = runs */
/* Test hook: the nth device allocation made from now on by a reconfiguration (m1v_reserve_scratch, m1v_set_pipelined, m1v_set_input_layout,
 * m1v_set_plane_layout, m1v_set_sample_layout, m1v_set_rgb_plane_layout, m1v_set_float_plane_layout, the m1v_debug_set_* hooks) fails as if the device were out of memory; 0 = off.  A failed reconfiguration returns
 * M1V_E_HIP and leaves the encoder exactly as it was.  Inert unless the process runs with EC504_DEBUG_HOOKS=1. */
void m1v_debug_fail_alloc(int nth);
/* Test hook: the next m1v_encode_device that reaches `stage` returns M1V_E_HIP there, as a failed HIP call would: 1 = after
 * the internal counter set is chosen, before the encode kernel; 2 = after the encode kernel (and the run layout), before
 * the assembly; 3 = after the assembly, before the pipelined completion event.  One-shot; 0 = off.  Host side only: it
 * launches nothing and touches no device memory.  Inert unless the process runs with EC504_DEBUG_HOOKS=1.  A size-table pass
 * of the tile path (m1v_frame_size_table_device, m1v_frame_rd_table_device, m1v_encode_rd_device, m1v_encode_budget_device, m1v_encode_batch_budget_device, m1v_encode_cbr_device)
 * reaches the stages as: 1 = before its probe kernel, 2 = after the probe kernel, before the sizes kernel, 3 = after the sizes
 * kernel. */
void m1v_debug_fail_encode(int stage);
/* Test hook: force how the RUN kernel loads its pixels (forcing a mode selects the run path): -1 = automatic (by width,
 * channel count and pointer alignment), 0 = byte loads (valid everywhere), 2 = 28-byte loads + funnel shift (3 channels,
 * 4-byte aligned buffer).  A mode that is not valid for the buffer at hand is ignored.  Lets tests compare the load paths
 * on one buffer. */
int m1v_debug_set_input_mode(m1v_encoder *enc, int mode);
/* Tuning/test hook: blocks per workgroup of the RUN kernel (multiple of 64, 64..384, not more than the blocks of one
 * strip; 0 = default).  Forcing a run length selects the run path unless m1v_debug_set_path says tiles. */
int m1v_debug_set_dense_threads(m1v_encoder *enc, int threads);
/* Test hook, read-only: the shape of the assembly kernel (k_assemble) under the plan in force.  out[0] = strips per workgroup
 * (1, 2, 4, 8 or 16), out[1] = log2 of the lanes that share a segment (1..4), out[2] = segments per strip (tile rows on the tile
 * path; the most runs a strip can touch on the run path; 1 for the strip kernel), out[3] = the producer: 0 = tiles, 1 = the run
 * kernel (dense), 2 = the strip kernel.  Launches nothing.  M1V_E_ARG for a null argument. */
int m1v_debug_assemble_shape(const m1v_encoder *enc, int out[4]);
/* Test hook: force that shape; 0 = the plan's own value, for either argument.  Every shape produces the same bytes: a group
 * whose bytes outgrow the kernel's LDS image takes several passes, one of more than 256 segments several chunks, a segment of
 * 4 * lanes words or more an extra loop.  Only values the plan can produce are taken: group a power of two, at most 16 and at
 * most m1v_strips(enc); lanes_log2 1..4.  Anything else returns M1V_E_ARG and changes nothing.  The forced values hold across
 * the other hooks and setters until they are set to 0.  A reconfiguration like the other m1v_debug_set_* hooks: it waits for
 * the device, and a failure leaves the encoder exactly as it was. */
int m1v_debug_set_assemble_shape(m1v_encoder *enc, int group, int lanes_log2);

#ifdef __cplusplus
}
#endif
#endif
