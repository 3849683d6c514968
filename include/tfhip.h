/*
 * tfhip.h -- C ABI of libtfhip.so: the MI355X (gfx950) backend for transflow's
 * per-frame hot loop (Farnebäck dense optical flow + compositor remap).
 *
 * This is the drop-in boundary.  Plain C types only: pointers,
 * sizes, POD structs.  Host pointers are borrowed for the duration of a call;
 * the library owns all device memory, tied to the opaque handles.  Every
 * function returns TF_OK (0) or a negative tf_status; the message of the last
 * failure on the calling thread is tf_last_error().  No HIP call happens at
 * load time: the first tf_init()/tf_*_create() initialises the runtime (the
 * reference runs the flow source in a forked child, pipeline.py:56-64).
 *
 * Each entry point cites the reference interface it replaces; paths are
 * relative to the reference tree (ychalier/transflow v1.11.1).
 */
#ifndef TFHIP_H
#define TFHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TFHIP_ABI_VERSION 1

typedef enum tf_status {
    TF_OK = 0,
    TF_ERR_ARG = -1,     /* bad argument (ValueError on the Python side) */
    TF_ERR_HIP = -2,     /* a HIP runtime call failed (RuntimeError) */
    TF_ERR_INDEX = -3,   /* a flow vector leaves the frame: the reference raises IndexError
                            at compositor/layers/movement.py:33,39 */
    TF_ERR_STATE = -4,   /* call order / handle state */
    TF_ERR_UNSUPPORTED = -5
} tf_status;

/* ---- runtime ------------------------------------------------------------------ */
int tf_abi_version(void);
/* Select the GPU for this process/thread and create the library stream.  Idempotent. */
int tf_init(int device);
/* 1 once this process has initialised the HIP runtime through the library (a process forked after
   that point cannot use the GPU: fork first, as transflow/pipeline.py does). */
int tf_is_initialized(void);
int tf_device_count(int *count);
/* Run-time options of the library (process-wide; defaults are the measured best):
     "fb_fused"       -1  the Farnebäck iteration as one kernel on levels of >= fb_fuse_min_px pixels over the
                          batch, as two kernels below; 0 = two kernels everywhere, 1 = one kernel wherever it
                          can run (read by tf_fb_create)
     "fb_fuse_min_px" 4000000
     "fb_no_share"    0   1 = pairs of a call that share a frame expand it once each (read per call)
     "fb_no_overlap"  0   1 = a call's kernels stay on the library stream (read by tf_fb_create)
     "remap_px"       4   pixels per thread of tf_remap_step_dev's kernel: 1, 2 or 4
     "remap_quad"     1   1 = with remap_px = 4, a frame width that is a multiple of 4 and 16-byte aligned buffers, a thread's
                          four pixels are adjacent ones of a row (16-byte loads and stores, the RGB frame stored from
                          registers); 0 = they are a block apart.  Same state and frames either way
     "remap_lean"     1   1 = where the step would take the adjacent-pixel kernel on the one-word state and the layer has no
                          source, destination or alpha mask, no reset_source, pixels_can_move_to_empty_spot and
                          _to_filled_spot on and no uniform field is supplied, it takes a kernel compiled for that
                          configuration (no run-time tests of it, 32-bit indices, one load per RGB pixel); 0 = the
                          general kernel.  Same state and frames
     "remap_no_pack"  0   0 = tf_remap_step_dev keeps the layer state as ONE 32-bit word per pixel between steps where row,
                          column, alpha and source index fit 13 + 13 + 1 + 5 bits (frames up to 8192 x 8192, 32
                          sources), as int16 x 4 otherwise; 2 = as int16 x 4 at most; 1 = as int32 x 4 (never packed)
     "remap_keep_rgba" 0  1 = tf_remap_steps_dev stores the layer's rgba in every step (it stores it in the last one alone where
                          every pixel is selected by source 0: nothing reads the others')
     "prof_levels"    0   1 = profiler labels carry the pyramid level
     "fb_exact_sums"  0   1 = the box window (flags without OPTFLOW_FARNEBACK_GAUSSIAN) is summed exactly as
                          FarnebackUpdateFlow_Blur sums it -- one set of running sums per image, float-differenced
                          down the columns from row 0, double-differenced along the rows from column 0 -- so the
                          flow is bit-identical to the CPU path's instead of within 1e-4 of it; about twice the
                          default's time, plus 40 bytes per pixel and pair of device memory (read per call)
     "fb_chain"       -1  the marching kernels keep FarnebackUpdateFlow_Blur's column sums (one running sum per column
                          from row 0).  A column cut into row segments needs the sum's value at each cut: 1 = every
                          segment waits for the one above it inside the launch (the sums are then the CPU path's bit
                          for bit), 0 = a pre-pass computes the values (equal up to the association of double
                          additions, ~1e-16), -1 = whichever is cheaper for the launch (read per call)
     "fb_segs"        0   > 0: that many row segments per column (0: chosen per launch; read per call)
     "jd_par_sub_bytes"  0  > 0: bytes of a subsequence of tf_jpegdec's parallel scan path, 16 to 1024 (0: the measured
                          best, 64; read per decode).  "jd_par_group_subs" 0: > 0: subsequences per work-group of that
                          path's synchronisation, 64, 128 or 256 (0: the measured best, 64; read per decode).
                          "jd_par_staged" 0: 1 = the synchronisation reads a work-group's share of the scan from LDS
                          where the subsequence is a power of two and the share fits 48 KB.  Test knobs
     "mt_segments"    0   > 0: the segments tf_mt_random_sample_dev cuts a field into, one wave each, up to 4096 (a
                          segment is never shorter than 256 words); 1 = one wave walks the field and no state ever
                          jumps; 0 = the measured default: one segment below 2^16 words, about 2^15 words a segment
                          above (read per draw: a change re-derives the segments' states).  Same doubles either way
   Unknown names and out-of-range values return TF_ERR_ARG.  The environment is never read. */
int tf_set_option(const char *name, long value);
int tf_get_option(const char *name, long *value);
const char *tf_last_error(void);
/* Block until everything queued on the library stream has finished. */
int tf_sync(void);
/* The hipStream_t all kernels of this library are launched on (for callers that
   record their own events or enqueue RCCL work in order with it). */
int tf_stream(void **hip_stream);

/* Events on the library stream (HIP events; bench.py times with these). */
typedef struct tf_event tf_event;
int tf_event_create(tf_event **ev);
int tf_event_record(tf_event *ev);
int tf_event_elapsed_ms(tf_event *start, tf_event *stop, float *ms); /* synchronises on stop */
void tf_event_destroy(tf_event *ev);
/* A flow that stays on the device between the flow source and the compositor (the seam transflow/pipeline.py:85-86,
   326, 562-567 crosses with a pickled host array): the producer records an event behind the flow's last kernel on ITS
   stream (tf_event_record), the consumer's stream waits for it on the device before its kernels read the flow
   (tf_stream_wait_event: no host synchronisation), or the host waits for it before the memory is handed to another
   process (tf_event_synchronize). */
int tf_stream_wait_event(tf_event *ev);
int tf_event_synchronize(tf_event *ev);
/* The same seam across the reference's process boundary (pipeline.py:56-64: the flow source is a child process, its
   items travel through a multiprocessing queue): a device allocation of this process (tf_dev_alloc) exported as 64
   opaque bytes (hipIpcGetMemHandle), opened in the consumer's process (hipIpcOpenMemHandle; one mapping per allocation,
   kept until tf_ipc_close) -- what crosses the queue is the 64 bytes instead of 66 MB per 4K flow.  The exporter
   keeps the allocation alive and untouched until the consumer has read it. */
#define TF_IPC_HANDLE_BYTES 64
int tf_ipc_export(void *dev, void *handle_out);
int tf_ipc_open(const void *handle, void **dev);
int tf_ipc_close(void *dev);

/* Per-kernel timing: when enabled every launch is bracketed by HIP events on the
   library stream.  tf_prof_report writes lines "name count total_ms" into buf. */
int tf_prof_enable(int on);
/* Only time kernels whose name contains `substring` (NULL or "" = all). */
int tf_prof_set_filter(const char *substring);
int tf_prof_reset(void);
int tf_prof_report(char *buf, size_t buf_size);

/* Page-locked host memory (hipHostMalloc): arrays the drop-in path hands across the boundary come from a pool of
   these, so that the copies behind tf_fb_get_flow / tf_comp_download (transflow/flow/sources/cv.py:490's result,
   transflow/output/ffmpeg.py:32-54's frame) and the upload of a flow into the compositor run at the link's rate
   instead of through the driver's staging of pageable memory. */
int tf_host_alloc(void **host, size_t bytes);
int tf_host_free(void *host);
/* The calling THREAD's library stream: 0 = the library stream (default), 1..3 = one of three further streams.
   Everything the thread then queues through the library -- uploads, a flow source's calls and downloads -- is ordered
   on that stream and runs beside other threads' work (the reference runs its flow source in a process of its own,
   transflow/pipeline.py:56-64; a prefetching flow source in a worker thread gets the same concurrency here). */
int tf_thread_stream(int which);

/* Raw device buffers, for harnesses that keep inputs resident in HBM. */
int tf_dev_alloc(void **dev, size_t bytes);
int tf_dev_free(void *dev);
int tf_dev_upload(void *dev, const void *host, size_t bytes);
int tf_dev_download(void *host, const void *dev, size_t bytes);
int tf_dev_copy(void *dst_dev, const void *src_dev, size_t bytes); /* device to device, on the library stream */
/* One 64-bit word stored at `dev` (8-byte aligned) in stream order on the calling thread's library stream: the
   generation word at the head of a flow buffer that crosses the reference's queue as an IPC token
   (transflow/pipeline.py:85-86, 326) -- bumped before the buffer is written again, compared by the consumer after
   its copy, so that a buffer rewritten too early raises instead of passing for the flow it no longer holds. */
int tf_dev_store_u64(void *dev, uint64_t value);
/* The same as one kernel, 16 bytes per lane: bench.py measures the practical HBM ceiling with it. */
int tf_dev_stream_copy(void *dst_dev, const void *src_dev, size_t bytes);

/* ---- Farnebäck dense optical flow ----------------------------------------------
 * Replaces cv2.calcOpticalFlowFarneback as called at
 * transflow/flow/sources/cv.py:479-490; parameter struct = the fb_* fields of
 * CvFlowConfig (cv.py:273-281).  flags (fb_flags, passed straight through at cv.py:489): 0 (transflow's
 * default), OPTFLOW_USE_INITIAL_FLOW = 4 (the flow array is read first: cv.py:478 fills it with the
 * previous output), OPTFLOW_FARNEBACK_GAUSSIAN = 256 (Gaussian instead of box window), or both.
 */
#define TF_OPTFLOW_USE_INITIAL_FLOW 4
#define TF_OPTFLOW_FARNEBACK_GAUSSIAN 256
typedef struct tf_fb_params {
    double pyr_scale;  /* fb_pyr_scale  (0.5)  */
    int levels;        /* fb_levels     (3)    */
    int winsize;       /* fb_winsize    (15)   */
    int iterations;    /* fb_iterations (3)    */
    int poly_n;        /* fb_poly_n     (5)    */
    double poly_sigma; /* fb_poly_sigma (1.2)  */
    int flags;         /* fb_flags      (0)    */
} tf_fb_params;

typedef struct tf_fb tf_fb;

/* frame_slots: how many uint8 grey frames the handle keeps resident in HBM;
   max_pairs: how many frame pairs one tf_fb_calc_slots call may process. */
int tf_fb_create(tf_fb **out, int width, int height, const tf_fb_params *params, int frame_slots, int max_pairs);
/* A second lane for first's calls (no counterpart in the reference, whose one call per frame is synchronous,
   cv.py:479-490): a handle of the same size and parameters that READS FIRST'S FRAME SLOTS and queues its calls on the
   library's other call stream.  Batches sent alternately to the two handles are in flight together, so the launches of
   one that leave the chip part-empty (coarse pyramid levels, the tail of every launch) run beside those of the other.
   Everything else is per handle: results are read from the handle that ran the call.  `first` destroyed while lanes
   still read its slots is released with the last of them (it must not be used after its own tf_fb_destroy).
   Not with tf_fb_keep_expansions.  A lane starts with first's tf_fb_set_exact mode. */
int tf_fb_create_lane(tf_fb **out, tf_fb *first);
void tf_fb_destroy(tf_fb *fb);
/* Which summation this HANDLE's calls use for the box window (cv.py:479-490: one call, one result; nothing outside
   the handle decides it): 1 = OpenCV's own order along the rows too (flow bit-identical to the CPU path's, ~2x the
   time), 0 = the default (window added across columns directly, every pixel within 1e-4 relative), -1 = whatever the
   process-wide option "fb_exact_sums" says when a call is issued (the state a new handle is in).  Takes effect with the
   next call; two handles of one process may differ, whichever threads drive them. */
int tf_fb_set_exact(tf_fb *fb, int mode);

/* One pair, host in / host out: flow_out is float32 [height][width][2] (x=dx, y=dy),
   exactly the array cv.py:479-490 produces.  Strides in bytes.  With TF_OPTFLOW_USE_INITIAL_FLOW the
   array is cv2's in/out `flow`: read as the initial flow, then overwritten with the result. */
int tf_fb_calc(tf_fb *fb, const uint8_t *prev, ptrdiff_t prev_stride, const uint8_t *next, ptrdiff_t next_stride,
               float *flow_out);

/* Resident path: upload grey frames into slots, compute n pairs in one pass
   (pairs are independent with flags == 0: cv.py:478,489), read results back or
   hand the device pointer on.  A slot named by several pairs of one call (consecutive pairs of a
   video share a frame) is expanded once for all of them; nothing is kept between calls.
   tf_fb_calc_slots only enqueues, on a stream of the library's
   own that does not wait for what the library stream was given last (the caller's remap of the
   previous result keeps running beside it), so a caller that fills frame slots on the device itself (through tf_fb_frame_ptr) calls tf_sync() before the next tf_fb_calc_slots;
   tf_fb_set_frame already returns with the frame in place. */
int tf_fb_set_frame(tf_fb *fb, int slot, const uint8_t *grey, ptrdiff_t stride);
/* The same from a decoded BGR frame, transflow/flow/sources/cv.py:461-466: uint8 [src_height][src_width][3]
   (row stride in bytes) is uploaded as it is and cv2.resize(INTER_NEAREST) to the handle's size +
   cv2.cvtColor(COLOR_BGR2GRAY) run on the device (tf_frame_grey_dev) straight into the slot. */
int tf_fb_set_frame_bgr(tf_fb *fb, int slot, const uint8_t *bgr, int src_width, int src_height, ptrdiff_t stride);
/* tf_fb_set_frame_bgr without the upload: bgr_dev is a complete, packed uint8 [src_height][src_width][3] frame in
   device memory (tf_jpegdec_decode_dev's output ...).  Ordered inside the library like the two above: it returns with
   the frame in place, so the caller needs no tf_sync(). */
int tf_fb_set_frame_bgr_dev(tf_fb *fb, int slot, const void *bgr_dev, int src_width, int src_height);
/* Resident path with TF_OPTFLOW_USE_INITIAL_FLOW: the initial flow of `pair` for the next tf_fb_calc_slots
   (float32 [height][width][2]; kept until written again, zero at creation), from the host or -- through
   its device address -- filled on the GPU (e.g. copied from a previous result, or left there as the chain state by
   tf_flow_post_process_chain_dev).  Ordering: tf_fb_calc_slots of such a handle waits, on the device, for everything
   the calling thread's library stream was given before the call, so a buffer filled by work queued on that stream
   needs no synchronise; work on any other stream the caller orders itself. */
int tf_fb_set_initial_flow(tf_fb *fb, int pair, const float *flow);
int tf_fb_initial_flow_ptr(tf_fb *fb, int pair, void **dev);
/* Streaming use (cv.py:460-490 holds prev_gray and reads one new frame per call): with `on`, the
   pyramid levels and polynomial expansion of a slot are kept from call to call and redone only
   after tf_fb_set_frame wrote the slot, so the frame that was "next" in one call costs nothing as
   "prev" in the following one.  Slots handed out by tf_fb_frame_ptr are expanded on every call.
   Needs frame_slots <= 2 * max_pairs.  Off by default: a call then depends on nothing but the frames. */
int tf_fb_keep_expansions(tf_fb *fb, int on);
int tf_fb_frame_ptr(tf_fb *fb, int slot, void **dev);
int tf_fb_calc_slots(tf_fb *fb, int n_pairs, const int *prev_slots, const int *next_slots);
int tf_fb_get_flow(tf_fb *fb, int pair, float *flow_out);
/* Streaming callers, one new frame and one flow per call (cv.py:460-490): with async io on, tf_fb_set_frame / _bgr put
   the frame up on a copy stream of the library's (they still return with the frame in place, but do not wait for the
   handle's kernels in flight), and tf_fb_get_flow_begin / _end bring the last call's flow down on another copy stream:
   _begin queues the copy behind what the caller's stream holds at that moment (its post_process), *token names the
   transfer; _end returns once flow_out is filled.  So frame t + 1 goes up and flow t - 1 comes down while pair t is being
   computed.  flow_out should be page-locked (tf_host_alloc) and stay untouched between _begin and _end. */
int tf_fb_async_io(tf_fb *fb, int on);
int tf_fb_get_flow_begin(tf_fb *fb, int pair, float *flow_out, int *token);
int tf_fb_get_flow_end(tf_fb *fb, int token);
int tf_fb_flow_ptr(tf_fb *fb, int pair, void **dev);

/* FlowSource.post_process (transflow/flow/sources/source.py:337-363) without the
   optional filter/mask/kernel pre-steps: direction 0 = FORWARD (clip, round,
   scatter-invert with last-write-wins, :349-360), 1 = BACKWARD; both end with the
   clip to the frame (:361-362).  In place. */
int tf_fb_post_process(tf_fb *fb, int pair, int direction);                 /* device flow of `pair` */
/* The first half of FORWARD post_process alone (source.py:349-358: clip, round, every moving source
   claims its target, the highest source index wins): *winners_dev = int32 [H][W], the winning source
   index per target or -1.  The handle owns the map; the next scatter or post_process overwrites it.
   tf_remap_step_dev(clip_flow = 2) takes it in place of the flow and does the rest (:359-362) in
   registers, which saves writing and re-reading the flow. */
int tf_fb_post_process_scatter(tf_fb *fb, int pair, void **winners_dev);
int tf_fb_post_process_host(tf_fb *fb, float *flow_inout, int direction);   /* host array, same H,W */

/* The optional pre-steps of post_process (source.py:339-345), applied before the direction
   handling: flow filters `scale`, `threshold`, `clip` (transflow/flow/filters.py:36-72) with the
   value the filter's lambda returned for this frame, then the flow mask multiply.  `wide` tells
   how numpy typed that value: 0 = Python float/int (NEP 50 weak scalar: arithmetic in float32),
   1 = numpy.float64 (arithmetic in float64, result cast to float32).  mask: float32 [H][W] or NULL. */
typedef enum tf_flow_op_kind { TF_FLOW_SCALE = 0, TF_FLOW_THRESHOLD = 1, TF_FLOW_CLIP = 2 } tf_flow_op_kind;
typedef struct tf_flow_op {
    int kind;
    int wide;
    double value;
} tf_flow_op;
#define TF_MAX_FLOW_OPS 8
int tf_fb_post_process_ex(tf_fb *fb, int pair, int direction, int n_ops, const tf_flow_op *ops, const void *mask_dev);
int tf_fb_post_process_host_ex(tf_fb *fb, float *flow_inout, int direction, int n_ops, const tf_flow_op *ops,
                               const float *mask); /* direction -1: pre-steps only */

/* ---- flow-array steps either side of the path (device pointers, no handle) ---------
 * Flows are float32 [H][W][2] unless `wide` says float64.  All launches go to the library stream. */

/* Pipeline.FLOW_MERGING_FUNCTIONS (transflow/pipeline.py:149-158; helpers transflow/utils.py:359-381):
   n flows of n_values floats each, combined left to right in float32 as numpy does. */
enum { TF_MERGE_FIRST = 0, TF_MERGE_SUM, TF_MERGE_AVERAGE, TF_MERGE_DIFFERENCE, TF_MERGE_PRODUCT, TF_MERGE_MASKBIN,
       TF_MERGE_MASKLIN, TF_MERGE_ABSMAX };
#define TF_MAX_MERGE 8
int tf_flow_merge_dev(int kind, int n, const void *const *flows_dev, void *out_dev, size_t n_values);

/* utils.upscale_array (utils.py:417-418): out [H*hf][W*wf][2] = (x*wf, y*hf) of the nearest source pixel. */
int tf_flow_upscale_dev(const void *in_dev, void *out_dev, int width, int height, int wf, int hf);

/* The two steps above in one pass, for flows that stay on the device (pipeline.py:502-504): n flows [height][width][2]
   merged by `kind`, then upscaled by the integer factors wf, hf >= 1 into out [height*hf][width*wf][2] -- bit for bit
   tf_flow_merge_dev followed by tf_flow_upscale_dev.  wf = hf = 1 is the merge alone, n = 1 with TF_MERGE_FIRST the
   upscale alone.  Pointers are 8-byte aligned; the output is stored 16 bytes a lane wherever its address allows.
   TF_ERR_ARG before any launch: a kind out of range, n outside 1..TF_MAX_MERGE, TF_MERGE_ABSMAX with n != 2, a factor
   below 1, a null pointer with a non-empty size, height*hf or width*wf beyond int.  An empty flow is a success. */
int tf_flow_seam_dev(int kind, int n, const void *const *flows_dev, int width, int height, int wf, int hf, void *out_dev);

/* The convolution-kernel pre-step of post_process (source.py:344-348):
   scipy.signal.convolve2d(channel, kernel, mode="same", boundary="fill", fillvalue=0) on both
   channels.  wide = 1: kernel float64 [kh][kw], out float64 [H][W][2] (numpy.result_type of a float32
   flow with a float64 or integer kernel); wide = 0: kernel and out float32. */
int tf_flow_convolve_dev(const void *flow_dev, const void *kernel_dev, int kh, int kw, int wide, void *out_dev, int width,
                         int height);

/* source.py:349-362 on a flow of either type, in place (after a convolution the reference carries
   on in the convolution's type).  FORWARD needs scratch_dev: 4 bytes per pixel. */
int tf_flow_post_process_dev(void *flow_dev, int wide, int width, int height, int direction, void *scratch_dev);
/* The whole of post_process short of the convolution, on a device flow and without a handle: the flow filters and the
   mask multiply (as tf_fb_post_process_ex: float32 flows only, wide with either is refused), then the direction
   handling; direction -1: none.  mask_dev: float32 [H][W] or NULL.  winner_dev: 4 bytes per pixel of the caller's,
   needed by FORWARD; it holds the winner map of tf_fb_post_process_scatter afterwards. */
int tf_flow_post_process_ex_dev(void *flow_dev, int wide, int width, int height, int direction, int n_ops,
                                const tf_flow_op *ops, const void *mask_dev, void *winner_dev);
/* The same on float32 flows, out of place, for a flow that sits in a method handle's own buffer (tf_hs_flow_ptr ...):
   src_dev is read once and left as it is (the handle writes it again on its next call); dst_dev receives exactly the
   bits tf_flow_post_process_ex_dev would leave in place.  chain_dev, where not NULL, receives what the reference's
   `prev_flow` holds after post_process (source.py:317, 337-363), the next call's initial flow: with a mask the flow
   after the filters and BEFORE the mask multiply (numpy.multiply makes a new array, which the direction handling and
   the clip then work on), without one the same bits as dst_dev.  Three distinct buffers of 8 bytes per pixel, 8-byte
   aligned.  BACKWARD and -1 are one launch, FORWARD a scatter and a resolve; no copy of the flow is made. */
int tf_flow_post_process_chain_dev(const void *src_dev, void *dst_dev, void *chain_dev, int width, int height,
                                   int direction, int n_ops, const tf_flow_op *ops, const void *mask_dev,
                                   void *winner_dev);
/* The convolution tail, source.py:344-362, out of place and without the intermediate array: src_dev (float32
   [H][W][2]) is left as it is, dst_dev (T [H][W][2]; T float64 with wide = 1, else float32, as is the kernel) receives
   exactly the bits tf_flow_convolve_dev followed by tf_flow_post_process_dev(wide, direction) would leave.  direction
   1 (BACKWARD) and -1 (the convolution alone) are one launch; 0 (FORWARD) is two: the convolution launch claims the
   targets in winner_dev (4 bytes per pixel, the caller's) and never stores the convolved flow, a resolve launch writes
   dst_dev.  Refused: null or aliased buffers, FORWARD without winner_dev, an empty kernel. */
int tf_flow_convolve_post_process_dev(const void *src_dev, const void *kernel_dev, int kh, int kw, int wide, void *dst_dev,
                                      int width, int height, int direction, void *winner_dev);
/* float32(rint(x)) (mode 0) or float32(floor(x)) (mode 1) of n_values float64 values, computed in double: what the
   compositor's layers make of a float64 flow (numpy.round, movement.py:21; numpy.floor, sum.py:10).  Ties go to even,
   -0.5 gives -0.0, NaN stays NaN.  src 8-byte and dst 4-byte aligned; both 16-byte aligned: two pixels a lane. */
int tf_flow_narrow_dev(const void *src_f64_dev, void *dst_f32_dev, size_t n_values, int mode);

/* The `polar` flow filter, transflow/flow/filters.py:75-87, in place on a float32 flow: r = |v|,
   a = atan2(vy, vx), then v = (R cos A, R sin A) with R and A the filter's two user expressions of
   (t, r, a).  The expressions arrive as postfix programs (transflow_amd/exprs.py compiles them; parts
   that are not arrays are evaluated on the host per frame and arrive as constants); a step computes in
   float32 unless `wide`, as numpy types the same expression.  wide_trig: sin/cos of A in float64;
   wide_product: the products in float64 (then cast to the float32 flow). */
typedef struct tf_polar_step {
    int op;      /* enum PolarOp of flowops.hip == index into transflow_amd/exprs.py OPS */
    int wide;
    double imm;  /* push_const only */
} tf_polar_step;
#define TF_MAX_POLAR_STEPS 48
#define TF_MAX_POLAR_STACK 12
int tf_flow_polar_dev(void *flow_dev, size_t n_pixels, int n_radius, const tf_polar_step *radius, int n_theta,
                      const tf_polar_step *theta, int wide_trig, int wide_product);

/* Flow visualisation, transflow/output/render.py:9-27 and :30-48: arr float32 [n] / flow float32
   [n][2] -> rgb uint8 [n][3].  colors_rgb: 2 (render1d) or 4 (render2d) colours as float triples. */
int tf_flow_render1d_dev(const void *arr_dev, void *rgb_dev, size_t n, float scale, const float colors_rgb[6], int binary);
int tf_flow_render2d_dev(const void *flow_dev, void *rgb_dev, size_t n, float scale, const float colors_rgb[12]);

/* The flow-magnitude view (pipeline.py:515-516): sqrt(x*x + y*y) of every vector of flow float32 [n_pixels][2], in
   float32 as numpy.sqrt(numpy.sum(numpy.power(flow, 2), axis=2)) computes it, straight into render1d's pixel rule:
   rgb uint8 [n_pixels][3] equals tf_flow_render1d_dev of that magnitude, which is never stored.  flow_dev is 8-byte,
   rgb_dev 4-byte aligned. */
int tf_flow_view_magnitude_dev(const void *flow_dev, void *rgb_dev, size_t n_pixels, float scale,
                               const float colors_rgb[6], int binary);

/* Frame ingest, transflow/flow/sources/cv.py:461-466: cv2.resize(INTER_NEAREST) to (width, height)
   then cv2.cvtColor(COLOR_BGR2GRAY), fused: bgr uint8 [src_height][src_width][3] -> grey uint8
   [height][width].  OpenCV's arithmetic is recalled, not verifiable here (parity unpinned). */
int tf_frame_grey_dev(const void *bgr_dev, int src_width, int src_height, void *grey_dev, int width, int height);

/* Stage-level entry points (debug/parity tests): run one stage of the pyramid on
   host arrays with exactly the kernels the full path uses.  Layouts as OpenCV's:
   R and M are [H][W][5] interleaved on the host side. */
int tf_fb_stage_level_image(tf_fb *fb, const uint8_t *grey, ptrdiff_t stride, int level, float *out /*[Hk][Wk]*/);
int tf_fb_stage_polyexp(tf_fb *fb, const float *img, int w, int h, float *r_out /*[h][w][5]*/);
/* A1 then A2 of one frame at one level, through whichever kernels the full path uses there
   (level 0 runs them fused): r_out [Hk][Wk][5]. */
int tf_fb_stage_level_polyexp(tf_fb *fb, const uint8_t *grey, ptrdiff_t stride, int level, float *r_out);
int tf_fb_stage_update_matrices(tf_fb *fb, const float *r0, const float *r1, const float *flow, int w, int h,
                                float *m_out /*[h][w][5]*/);
/* A5 then A3 at `level` (0 <= level < K) as the pyramid runs them: coarse_flow [Hc][Wc][2] of level + 1 is
   upsampled (resize INTER_LINEAR to the level's size, times 1/pyr_scale) inside the matrix kernel. */
int tf_fb_stage_upsampled_matrices(tf_fb *fb, int level, const float *r0, const float *r1, const float *coarse_flow,
                                   float *m_out /*[Hk][Wk][5]*/);
/* A4: the box window (FarnebackUpdateFlow_Blur) -- or, on a handle with TF_OPTFLOW_FARNEBACK_GAUSSIAN, the
   Gaussian one (FarnebackUpdateFlow_GaussianBlur) -- and the 2x2 solve. */
int tf_fb_stage_blur_solve(tf_fb *fb, const float *m, int w, int h, float *flow_out /*[h][w][2]*/);
/* The first step of TF_OPTFLOW_USE_INITIAL_FLOW: flow [H][W][2] -> [Hc][Wc][2] of the coarsest scale,
   resize(INTER_AREA) times pyr_scale^K. */
int tf_fb_stage_initial_flow(tf_fb *fb, const float *flow, float *coarse_out);
int tf_fb_level_count(tf_fb *fb, int *n_scales); /* K+1 */
int tf_fb_level_size(tf_fb *fb, int level, int *w, int *h);

/* ---- Horn-Schunck (transflow/flow/methods/horn_schunck.py) ------------------------
 * calc_optical_flow_horn_schunck(prev, next, flow, alpha, max_iters, decay, delta), bit for bit, for up to
 * max_pairs (<= 64) frame pairs per call.  Frame slots as tf_fb's.  A pair with an initial flow
 * (tf_hs_set_initial_flow) runs the float32 chain from u = decay * flow; one without runs the float64 chain
 * from zeros (the reference's flow=None).  The convergence test sigma_max(u - u_prev) < delta is decided on the
 * device when it can be, with a relative guard of 1e-3 (cheap bounds, power iteration, a Gram certificate);
 * otherwise the pair WAITS: the caller downloads du (tf_hs_delta_download), evaluates numpy.linalg.norm(du, 2) <
 * delta itself, reports it (tf_hs_resolve) and calls tf_hs_resume.  tf_hs_calc_slots / tf_hs_resume return
 * once every pair is done or waiting; tf_hs_waiting says which wait (n = 0: the flows are ready). */
typedef struct tf_hs_params {
    double alpha_sq;   /* alpha ** 2 as Python evaluates it; rounded to float32 in the denominator */
    double decay;      /* rounded to float32: u = decay * flow[..., 0] */
    int max_iters;     /* <= 0: the initial field */
    double delta;
    int has_delta;     /* 0: delta is None, every call runs max_iters iterations */
} tf_hs_params;
typedef struct tf_hs tf_hs;
int tf_hs_create(tf_hs **out, int width, int height, int frame_slots, int max_pairs);
void tf_hs_destroy(tf_hs *hs);
int tf_hs_set_frame(tf_hs *hs, int slot, const uint8_t *grey, ptrdiff_t stride);
int tf_hs_set_frame_bgr(tf_hs *hs, int slot, const uint8_t *bgr, int src_width, int src_height, ptrdiff_t stride);
/* flow [H][W][2] float32 for the next call's `pair`, or NULL: the float64 chain.  Read by the next call only. */
int tf_hs_set_initial_flow(tf_hs *hs, int pair, const float *flow);
/* The same from a device address (NULL: the float64 chain), without a copy and without synchronising the host: the
   pointer is BORROWED.  The next tf_hs_calc_slots reads it once, in its first kernel of the pair, on the calling
   thread's stream; work queued on that stream after the call may write the buffer again (a chain buffer that
   tf_flow_post_process_chain_dev fills after every call is the intended use). */
int tf_hs_set_initial_flow_dev(tf_hs *hs, int pair, const void *flow_dev);
int tf_hs_calc_slots(tf_hs *hs, const tf_hs_params *params, int n_pairs, const int *prev_slots, const int *next_slots);
int tf_hs_waiting(tf_hs *hs, int *pairs_out /* [max_pairs] */, int *n_waiting);
/* du = u - u_prev of a waiting pair: [H][W] float64 (*is_f64 = 1) or float32 */
int tf_hs_delta_download(tf_hs *hs, int pair, void *out, int *is_f64);
int tf_hs_resolve(tf_hs *hs, int pair, int converged);
int tf_hs_resume(tf_hs *hs);
int tf_hs_get_flow(tf_hs *hs, int pair, float *flow_out /* [H][W][2] */);
int tf_hs_flow_ptr(tf_hs *hs, int pair, void **dev);
/* stats[5] of `pair` in the last call: iterations run, then how many convergence decisions each stage made:
   cheap bounds, power iteration, Gram certificate, host */
int tf_hs_stats(tf_hs *hs, int pair, int *stats);
/* The prepare kernel alone: out [H][W][4] float32 {ex, ey, et, alpha_sq + ex^2 + ey^2} */
int tf_hs_stage_derivatives(tf_hs *hs, const uint8_t *prev, const uint8_t *next, double alpha_sq, float *out);
/* The device stages of the convergence test on a host field du [h][w] (float64 if is_f64, else float32):
   *decision 1 (sigma_max < delta), 0 (not), -1 (the host must decide); *stage 0 bounds, 1 power, 2 Gram, 3 host. */
int tf_hs_stage_norm_test(const void *field, int w, int h, int is_f64, double delta, int *decision, int *stage);
/* Every stage of that test without early exit, on du = u_new - u_old taken in the fields' type (u_old NULL: zeros):
   out[3 + 16 + 3] = F, U, L of the cheap bounds; the 16 lower bounds of the 8 power-iteration steps (||du x||, then
   ||du^T y||, per step); the Gram bounds of k = 1, 2, 4.  The stages after the bounds run through the host code of
   the decision path; where that path does not run them (du not finite, or ||du||_F^2 below 2^-960) their values are
   NaN, as are the Gram bounds when F is 0. */
int tf_hs_stage_norm_values(const void *u_new, const void *u_old, int w, int h, int is_f64, double *out);
/* out[3] = F, U, L of `pair`'s most recent convergence check in the last call, from the partial sums that the
   iteration kernel wrote.  TF_ERR_ARG when that call made none for the pair (no delta, or no iteration). */
int tf_hs_stage_last_bounds(tf_hs *hs, int pair, double *out);

/* ---- Lucas-Kanade (transflow/flow/methods/lukas_kanade.py) ---------------------------
 * calc_optical_flow_lukas_kanade(prev, next, win_size, max_level, step): cv2.calcOpticalFlowPyrLK over the grid
 * arange(0, W, step) x arange(0, H, step) with the default criteria and flags, flow = nextPts - p0 whatever the
 * status, block-replicated to step x step and cropped to H x W: a float32 [H][W][2] per pair, for up to max_pairs
 * (<= 64) pairs per call.  Bit for bit with the numpy restatement tests/lk_ref.py.  Frame slots as tf_fb's: a slot
 * keeps its pyramid (and, as a prev frame, its derivatives) until set_frame or a call with another win_size /
 * level count.  collect_stats: count the steps run per point and level (tf_lk_stats). */
#define TF_LK_MAX_LEVELS 20
typedef struct tf_lk tf_lk;
int tf_lk_create(tf_lk **out, int width, int height, int frame_slots, int max_pairs);
void tf_lk_destroy(tf_lk *lk);
int tf_lk_set_frame(tf_lk *lk, int slot, const uint8_t *grey, ptrdiff_t stride);
int tf_lk_set_frame_bgr(tf_lk *lk, int slot, const uint8_t *bgr, int src_width, int src_height, ptrdiff_t stride);
int tf_lk_calc_slots(tf_lk *lk, int win_size, int max_level, int step, int n_pairs, const int *prev_slots,
                     const int *next_slots, int collect_stats);
int tf_lk_get_flow(tf_lk *lk, int pair, float *flow_out /* [H][W][2] */);
int tf_lk_flow_ptr(tf_lk *lk, int pair, void **dev);
/* Of the last call (zeros unless it collected them): *n_levels, and sum_max[TF_LK_MAX_LEVELS][2] = {sum, max} over
   the points of the steps run at each level */
int tf_lk_stats(tf_lk *lk, int pair, int *n_levels, unsigned long long *sum_max);
/* Stage entry points.  A pyramid level of a slot, padded by win_size with reflect-101: uint8 [h+2w][w+2w]; the Scharr
   derivatives of one, zero-padded: int16 [h+2w][w+2w][2] {dx, dy}; one point's trace: out[level][4] = {nextPts.x,
   nextPts.y, steps run, code (0 done, 1 lost at the prev bounds, 2 at the eigenvalue test, 3 at the next bounds)}
   after each level, for levels 0 .. the pyramid's count. */
int tf_lk_stage_pyramid(tf_lk *lk, int slot, int win_size, int max_level, int level, uint8_t *out);
int tf_lk_stage_scharr(tf_lk *lk, int slot, int win_size, int max_level, int level, int16_t *out);
int tf_lk_stage_trace(tf_lk *lk, int prev_slot, int next_slot, int win_size, int max_level, float x, float y, float *out);

/* ---- LiteFlowNet (transflow/flow/methods/liteflownet.py) ------------------------------
 * calc_optical_flow_liteflownet(prev, next) of cv.py:509-516: the network on the pair's BGR frames (x 1/255, bilinear
 * to Hp x Wp = W, H rounded up to multiples of 32, the per-role mean subtracted), the flow x 20 resized back to W x H
 * and scaled by W / Wp, H / Hp: a float32 [H][W][2] per pair, for up to max_pairs (<= TF_LFN_MAX_PAIRS) pairs per
 * call, all batched.  Float32 throughout in the default precision; the convolutions sum in their own order, the
 * correlation in the reference's (tests/lfn_ref.py).  tf_lfn_set_precision chooses, per handle, how the network's
 * convolutions (and nothing else: netScaleX/Y, the correlation, the transposed convs, backwarp and the resizes never
 * change) multiply.  With q(v) = v rounded to bfloat16, ties to even:
 *   TF_LFN_F32     sum x w + b in float32 (the default)
 *   TF_LFN_BF16    sum q(x) q(w) + b: activations are rounded where a convolution reads them (they stay float32 in
 *                  memory), weights once; products are exact in float32, sums, bias, LeakyReLU and residual float32
 *   TF_LFN_BF16X3  with xh = q(x), xl = q(x - xh), wh = q(w), wl = q(w - wh):
 *                  sum (xh wh + xh wl + xl wh) + b, one float32 chain over K ascending that takes, for each step of
 *                  16 k, xh wh, then xh wl, then xl wh
 * The mode may be set before or after the weights and between calls; another value is TF_ERR_ARG and the handle keeps
 * its mode.  Every mode is bit-identical from run to run and for a pair alone or in a batch.  The weights are the
 * caller's: tf_lfn_set_weights takes every layer's weight and bias as one float32 blob in the order of
 * transflow_amd/liteflownet.py param_spec() and repacks them on the device.  W and H must exceed 32 (at 32 or less the
 * reference divides by zero in its backwarp).  A frame slot holds the frame (uint8 BGR, W x H); nothing computed from
 * it is kept between calls (a frame's features depend on its role). */
#define TF_LFN_MAX_PAIRS 16
typedef struct tf_lfn tf_lfn;
int tf_lfn_create(tf_lfn **out, int width, int height, int frame_slots, int max_pairs);
void tf_lfn_destroy(tf_lfn *lfn);
int tf_lfn_set_weights(tf_lfn *lfn, const float *blob, long long n_floats);
#define TF_LFN_F32 0
#define TF_LFN_BF16 1
#define TF_LFN_BF16X3 2
int tf_lfn_set_precision(tf_lfn *lfn, int precision);
int tf_lfn_get_precision(tf_lfn *lfn, int *precision);
int tf_lfn_set_frame_bgr(tf_lfn *lfn, int slot, const uint8_t *bgr, int src_width, int src_height, ptrdiff_t stride);
int tf_lfn_calc_slots(tf_lfn *lfn, int n_pairs, const int *prev_slots, const int *next_slots);
int tf_lfn_get_flow(tf_lfn *lfn, int pair, float *flow_out /* [H][W][2] */);
int tf_lfn_flow_ptr(tf_lfn *lfn, int pair, void **dev);
/* Stage entry points, host arrays in and out, activations NHWC float32.  conv: layer `layer` of param_spec's layer
   list on n images h x w, its Cin input channels at in_off of in_cs, written at out_off of out_cs (the other channels
   of out are kept), plus the residual at res_off of res_cs when res is not null; bias and LeakyReLU as the layer has
   them, in the handle's precision.  deconv: a depthwise 4x4 stride-2 transposed conv [n][h][w][C] -> [n][2h][2w][C].
   correlation: LeakyReLU(correlation) [n][ceil(h/s)][ceil(w/s)][49].  backwarp: in [n][h][w][c] at flow [n][h][w][2]
   x scale.  regularize_tail: the level's -d^2 / softmax / netScaleX, Y / divisor on dist [n][h][w][k^2] and flow
   [n][h][w][2].  prep: a slot's frame in role 0 (one) or 1 (two), [Hp][Wp][3]. */
int tf_lfn_stage_conv(tf_lfn *lfn, int layer, int n, int h, int w, const float *in, int in_cs, int in_off,
                      const float *res, int res_cs, int res_off, float *out, int out_cs, int out_off);
int tf_lfn_stage_deconv(tf_lfn *lfn, int layer, int n, int h, int w, const float *in, float *out);
int tf_lfn_stage_correlation(tf_lfn *lfn, int stride, int n, int h, int w, int c, const float *one, const float *two,
                             float *out);
int tf_lfn_stage_backwarp(tf_lfn *lfn, int n, int h, int w, int c, const float *in, const float *flow, float scale,
                          float *out);
int tf_lfn_stage_regularize_tail(tf_lfn *lfn, int level, int n, int h, int w, const float *dist, const float *flow,
                                 float *out);
int tf_lfn_stage_prep(tf_lfn *lfn, int slot, int role, float *out);

/* ---- codec motion vectors (transflow/flow/sources/av.py) -------------------------------
 * AvFlowSource.next() (av.py:61-77): flow = zeros [H][W][2] float32; then, for each vector in list order,
 *   flow[src_y - h//2 : src_y + h//2, src_x - w//2 : src_x + w//2] = -motion_x / motion_scale, -motion_y / motion_scale
 * with numpy's slice semantics (a negative bound counts from the end, then both clamp to [0, n]: rectangles near the
 * top or left edge wrap, they are not clipped), float64 quotients rounded to float32 on assignment (motion 0 paints
 * -0.0) and the last writer of a pixel winning.  The entries take the RAW fields of libavutil's AVMotionVector and do
 * the slice resolution, the division and the checks themselves.  A vector with source != -1 (the assert of av.py:69)
 * or motion_scale == 0 (the ZeroDivisionError of av.py:74) is TF_ERR_ARG, the message names its index, and nothing
 * is launched.  n == 0 (v may be null then; a frame without MOTION_VECTORS side data, av.py:66-67) gives all +0.0.
 * A tf_mv belongs to one calling thread: its upload stage and event are the handle's, the stream is the thread's. */
typedef struct tf_mv_vector {
    int32_t source, w, h, src_x, src_y, motion_x, motion_y, motion_scale;
} tf_mv_vector;
typedef struct tf_mv tf_mv;
int tf_mv_create(tf_mv **out, int width, int height);
void tf_mv_destroy(tf_mv *mv);
/* av.py:62-77 for one frame, into a host array ... */
int tf_mv_rasterize(tf_mv *mv, const tf_mv_vector *v, int n, float *flow_out /* host [H][W][2] */);
/* ... or into device memory (8-byte aligned), queued on the calling thread's stream: nothing is waited for */
int tf_mv_rasterize_dev(tf_mv *mv, const tf_mv_vector *v, int n, void *flow_dev /* device [H][W][2] */);
/* Stage entry point, host arithmetic only (no device needed): av.py:70-75 per vector.  rects_out[k] = {i0, i1, j0, j1}
   after the slice resolution (rows [i0, i1) x columns [j0, j1); empty when i0 >= i1 or j0 >= j1), values_out[k] =
   {float32(-dx), float32(-dy)}. */
int tf_mv_stage_resolve_rects(int width, int height, const tf_mv_vector *v, int n, int32_t *rects_out /* n x 4 */,
                              float *values_out /* n x 2 */);

/* ---- still pixmaps generated where they are read (transflow/pixmap/still.py) -------------
 * The image whose pixels the layers move, uint8 [H][W][3] in device memory the caller owns (4-byte aligned), for
 * tf_remap_gather_dev / tf_remap_introduce_dev / tf_remap_step_dev to read.  Both calls queue on the calling thread's
 * stream and wait for nothing.
 * tf_pixmap_fill_dev: ColorPixmapSource._init_array (still.py:52-53), every pixel the one colour.
 * tf_pixmap_gradient_dev: GradientPixmapSource.evaluate + _init_array (still.py:121-163) for every pixel of an
 * expression tree given in postfix order (children before their parent, the root last).  In float64, one rounding
 * per Python operation:
 *   TF_PX_I       z = 2 * (i / (height - 1)) - 1 in all three channels     TF_PX_J  the same with j and width
 *   TF_PX_RGB     (a, b, c)
 *   TF_PX_MIX     of the three values A, B, C below it, per channel k: w = (1 + A[k]) / 2; (1 - w) * B[k] + w * C[k]
 *   TF_PX_TRIPLE  (A[0], B[1], C[2])
 *   the byte of a channel v: (255 * (v + 1)) / 2, truncated toward zero to a 32-bit integer, its low 8 bits.
 * The trees still.py:94-119 generates have one shape -- a triple of three slots, each a leaf or a mix of three slots,
 * each of those a leaf or a mix of three leaves: at most 40 nodes -- and that shape is what the kernel evaluates, with
 * every register index a constant.  A root that is not a triple R is taken as the triple (R, R, R), which has the same
 * value.  TF_ERR_ARG, and nothing launched: more than TF_PX_MAX_NODES nodes, an unknown type, a postfix order that does
 * not reduce to one tree, TF_PX_I with height 1 or TF_PX_J with width 1 (the reference's ZeroDivisionError).
 * TF_ERR_UNSUPPORTED, and nothing launched: a well-formed tree of another shape (a triple below the root, mixes nested
 * three deep). */
enum { TF_PX_I = 0, TF_PX_J = 1, TF_PX_RGB = 2, TF_PX_MIX = 3, TF_PX_TRIPLE = 4 };
#define TF_PX_MAX_NODES 40
typedef struct tf_px_node {
    int type;
    double a, b, c; /* TF_PX_RGB's channels; ignored for the other types */
} tf_px_node;
int tf_pixmap_fill_dev(void *rgb_dev, size_t n_pixels, const uint8_t rgb[3]);
int tf_pixmap_gradient_dev(void *rgb_dev, int width, int height, int n_nodes, const tf_px_node *nodes);

/* ---- compositor layers -----------------------------------------------------------
 * One handle = one layer of the compositor.  layer_class selects which of the reference's
 * layer classes it is (Layer.from_args, transflow/compositor/layers/layer.py:44-56):
 *   TF_LAYER_MOVEREF       MoveReferenceLayer (move_reference.py:6-14): MovementLayer.update
 *                          (movement.py:20-64) then ReferenceLayer.update (reference.py:58-109)
 *   TF_LAYER_SUM           SumLayer (sum.py:7-14): (i, j) += floor(flow), then ReferenceLayer.update
 *   TF_LAYER_STATIC        StaticLayer (static.py:7-17): pixmaps copied where introduced
 *   TF_LAYER_INTRODUCTION  IntroductionLayer (introduction.py:8-73): 8-channel canvas
 *                          (r, g, b, alpha, source, i, j, frame), moved by the flow, then fed
 * and Layer.render (layer.py:32-34) for all of them.  tf_layer_cfg carries the LayerConfig
 * fields the layers read (transflow/config.py:88-105).
 */
enum { TF_LAYER_MOVEREF = 0, TF_LAYER_SUM = 1, TF_LAYER_STATIC = 2, TF_LAYER_INTRODUCTION = 3 };

typedef struct tf_layer_cfg {
    int transparent_pixels_can_move;    /* False */
    int pixels_can_move_to_empty_spot;  /* True  */
    int pixels_can_move_to_filled_spot; /* True  */
    int moving_pixels_leave_empty_spot; /* False */
    int reset_mode;                     /* 0 off, 1 random, 2 constant, 3 linear (reference.py:16-21) */
    double reset_random_factor;         /* 1   */
    double reset_constant_step;         /* 1   */
    double reset_linear_factor;         /* 0.1 */
    int reset_source;                   /* False */
    int layer_class;                    /* TF_LAYER_*; 0 = moveref */
    /* introduction.py:24-44.  As the reference is written, on_empty_spots, unmoving_pixels and
       the mask write of on_all_empty_spots index with the Python value False and select nothing;
       they are carried for completeness, on_all_empty_spots still turns `consider_flow` off (:40). */
    int introduce_pixels_on_empty_spots;  /* True  (no effect) */
    int introduce_pixels_on_filled_spots; /* True  */
    int introduce_moving_pixels;          /* True  */
    int introduce_unmoving_pixels;        /* True  (no effect) */
    int introduce_on_all_filled_spots;    /* False */
    int introduce_on_all_empty_spots;     /* False */
} tf_layer_cfg;

typedef struct tf_remap tf_remap;
typedef struct tf_comp tf_comp;

/* Masks are [height][width]; NULL = the reference's default (mask_src/mask_dst all
   true, mask_alpha/reset_mask all 1.0: layer.py:24, movement.py:14-15, reference.py:44).
   moveref/sum: data starts as (i, j, 1, 0) per pixel (reference.py:40-42); introduction: an
   all-zero 8-channel canvas (data.py:17); static: no data, rgba alpha = 1 (static.py:11). */
int tf_remap_create(tf_remap **out, int height, int width, const tf_layer_cfg *cfg, const uint8_t *mask_src,
                    const uint8_t *mask_dst, const float *mask_alpha, const float *reset_mask);
void tf_remap_destroy(tf_remap *layer);

/* ReferenceLayer.set_sources (reference.py:54-56): remembers the introduction masks
   (uint8 [height][width] each) and writes source index s where mask s is set. */
int tf_remap_set_sources(tf_remap *layer, int n_sources, const uint8_t *const *introduction_masks);

/* The flow-dependent part of Layer.update.  moveref: MovementLayer.update +
   ReferenceLayer._update_reset; sum: the accumulation (sum.py:10) + _update_reset;
   introduction: MovementLayer.update on the 8-channel canvas and the introduction mask
   (introduction.py:24-44) for the tf_remap_introduce calls that follow; static: nothing
   (static.py:13 ignores the flow).  `flow` float32 [H][W][2]
   (already post-processed).  `uniform`: float64 [H][W] in [0,1) -- the field the
   reference draws with numpy.random.random (reference.py:59) -- or NULL to draw it
   on the GPU from `seed` and the handle's frame counter.  Returns TF_ERR_INDEX if a
   rounded flow vector leaves the frame (state is then unchanged). */
int tf_remap_update(tf_remap *layer, const float *flow, const double *uniform, uint64_t seed);
int tf_remap_update_dev(tf_remap *layer, const void *flow_dev, const void *uniform_dev, uint64_t seed);
/* The float64 [H][W] field the NEXT tf_remap_update(_dev) / tf_remap_step_dev call on this layer would
   draw for uniform == NULL with this seed (it depends on the seed, the pixel and the layer's frame
   counter): written to uniform_dev so that a checker can hand the very same field to a CPU statement
   of reference.py:58-67 -- on-GPU draws are then comparable bit for bit. */
int tf_remap_uniform_dev(tf_remap *layer, uint64_t seed, void *uniform_dev);
/* Deferred form of the range check for the resident path: 1 if any update_dev since
   the last call saw an out-of-frame vector (those updates were skipped). */
int tf_remap_check(tf_remap *layer, int *out_of_frame);

/* One iteration of the per-source loop for source `source_index`; pixmap is uint8
   [H][W][channels], channels 3 or 4.  moveref/sum: ReferenceLayer._update_rgba
   (reference.py:94-105); static: the masked copy of static.py:14-17. */
int tf_remap_gather(tf_remap *layer, int source_index, const uint8_t *pixmap, int channels);
int tf_remap_gather_dev(tf_remap *layer, int source_index, const void *pixmap_dev, int channels);
/* tf_remap_gather with the pixmap going up on the library's upload stream, beside whatever the caller queued before it
   (the same iteration of reference.py:94-105 / static.py:14-17; the call still returns with the host pixmap consumed):
   for an update whose flow was on the device already (transflow/pipeline.py:562-567 with a DeviceFlow), where the
   upload would otherwise wait for the update kernel. */
int tf_remap_gather_beside(tf_remap *layer, int source_index, const uint8_t *pixmap, int channels);
/* The upload alone: the pixmap of `source.next()` (reference.py:99) into the layer's staging buffer -- on the library's
   upload stream if `beside` -- for a caller that runs the frame's kernels later in one launch (tf_remap_step_dev with
   *pixmap_dev: HipCompositor does, between update() and render(), compositor.py:27-40).  Returns with the host pixmap
   consumed.  tf_remap_staged_used: call after queueing the last kernel that reads the staging buffer (the next
   upload waits for it on the device). */
int tf_remap_stage_pixmap(tf_remap *layer, const uint8_t *pixmap, int channels, int beside, void **pixmap_dev);
int tf_remap_staged_used(tf_remap *layer);

/* Introduction layer: one iteration of introduction.py:46-63 -- every target selected by the
   mask tf_remap_update left and by the source's introduction mask takes the record
   (pixmap[s], [1 if RGB], source_index, i(s), j(s), frame_number) of s = target + rounded flow
   (s = target when an introduce_on_all_* flag is set).  introduce_once is the caller's business
   (introduction.py:21-23 returns before the sources are even asked for a frame). */
int tf_remap_introduce(tf_remap *layer, int source_index, const uint8_t *pixmap, int channels, int frame_number);
int tf_remap_introduce_dev(tf_remap *layer, int source_index, const void *pixmap_dev, int channels, int frame_number);

/* Layer.render (layer.py:32-34) + this layer's turn in Compositor.render
   (compositor.py:36-39): alpha := uint8(mask_alpha*alpha) in place, then paint the
   opaque pixels onto the compositor image. */
int tf_remap_render(tf_remap *layer, tf_comp *comp);

/* The resident path's one call per frame, same result as
     [clip of post_process BACKWARD on the flow, if clip_flow]; tf_remap_update_dev;
     tf_remap_gather_dev(source 0); tf_comp_begin; tf_remap_render
   for a compositor with this single layer and a single source.  Runs as ONE kernel when
   the layer needs no second pass (moving_pixels_leave_empty_spot off, reset off/random),
   otherwise as those separate kernels.  clip_flow: 0 = flow_dev is a post-processed flow; 1 = clip it
   first (BACKWARD post_process is the clip alone; written back only in the unfused form, the fused
   form clips in registers); 2 = flow_dev is the winner map of tf_fb_post_process_scatter, the flow
   it stands for (source.py:359-362) is formed in registers. */
int tf_remap_step_dev(tf_remap *layer, tf_comp *comp, const void *flow_dev, int clip_flow, const void *uniform_dev,
                      uint64_t seed, const void *pixmap_dev, int channels);
/* n consecutive tf_remap_step_dev calls as one: step i takes flows_dev[i], paints comps[i] from pixmaps_dev[i] and
   draws from uniforms_dev[i] (uniforms_dev NULL: the generator, as a NULL uniform_dev above).  The layer state and the n
   frames are those of the n calls (pipeline.py:565 + :518 for n consecutive flows of a clip whose frames stay on
   the device).  Knowing the steps that follow, the call leaves out stores nothing reads: while every pixel is
   selected by source 0 -- checked on the device before the first step; a one-source moveref layer that takes the
   one-kernel step keeps it so -- a step's rgba (reference.py:93-105) is overwritten whole by the next step without
   having been read, so only the last step stores it (option "remap_keep_rgba" = 1 stores it every time). */
int tf_remap_steps_dev(tf_remap *layer, int n, tf_comp *const *comps, const void *const *flows_dev, int clip_flow,
                       const void *const *uniforms_dev, uint64_t seed, const void *const *pixmaps_dev, int channels);

/* State exchange for checkpoints (pipeline.py:225-242 pickles the compositor) and
   for extra/control.py:146-162 which reads layer.data.  data int32 [H][W][4]
   (i, j, alpha, source) -- [H][W][8] for an introduction layer, absent for a static one;
   rgba uint8 [H][W][4] (an introduction layer's rgba IS data[..., :4]: pass NULL).
   Either pointer may be NULL.  tf_remap_data_depth: 4, 8 or 0. */
int tf_remap_data_depth(tf_remap *layer, int *depth);
int tf_remap_get_state(tf_remap *layer, int32_t *data, uint8_t *rgba);
int tf_remap_set_state(tf_remap *layer, const int32_t *data, const uint8_t *rgba);

/* Compositor image (compositor.py:17-40): background colour + output frame. */
int tf_comp_create(tf_comp **out, int height, int width, const uint8_t background_rgb[3]);
/* The same with the image in the caller's device memory (H*W*3 bytes at image_dev, which must outlive
   the handle): the frames of a batch side by side in one buffer are what one tf_batch_gather sends
   (pipeline.py:518 hands every finished frame to one output). */
int tf_comp_create_on(tf_comp **out, int height, int width, const uint8_t background_rgb[3], void *image_dev);
void tf_comp_destroy(tf_comp *comp);
int tf_comp_begin(tf_comp *comp);                      /* image = background.copy() (:35) */
int tf_comp_download(tf_comp *comp, uint8_t *rgb_out); /* uint8 [H][W][3] (:40) */
/* The same download beside whatever the caller queues next (pipeline.py:518 hands the frame to the outputs' queue,
   pipeline.py:565 goes on to the next update; output/ffmpeg.py:32-54 writes it to the encoder's pipe): the copy starts
   when the caller's stream reaches this point, on the library's download stream; tf_comp_download_end returns once
   rgb_out (page-locked: tf_host_alloc) is filled.  The image must not be written again before _end: a caller that
   wants frame t on its way down while it renders frame t + 1 alternates two images.  _end without _begin: no-op. */
int tf_comp_download_begin(tf_comp *comp, uint8_t *rgb_out);
int tf_comp_download_end(tf_comp *comp);
int tf_comp_image_ptr(tf_comp *comp, void **dev);

/* ---- baseline JPEG of a frame in device memory (transflow/output/mjpeg.py:58-60, output/frames.py: the outputs whose
 * product is a compressed frame) --------------------------------------------------------------------------------------
 * The file libjpeg writes for 8-bit YCbCr 4:2:0 (sampling 2x2, 1x1, 1x1), one interleaved scan, the Annex K Huffman
 * tables, the tables of jpeg_set_quality(quality, force_baseline) and a restart interval of `restart_mcus` MCUs --
 * Pillow's save(quality=q, subsampling=2, restart_marker_blocks=r), byte for byte.  The restart intervals are coded
 * side by side on the device; every decoder reproduces the pixels of the file without them.
 * restart_mcus: 1 to 65535, 0 = the library's default.  The handle owns the header (SOI, JFIF APP0, two DQT, SOF0,
 * four DHT, DRI, SOS: made once) and its staging, scan and packed-stream buffers, sized for the worst case at creation. */
typedef struct tf_jpeg tf_jpeg;
int tf_jpeg_create(tf_jpeg **out, int height, int width, int quality, int restart_mcus);
void tf_jpeg_destroy(tf_jpeg *enc);
int tf_jpeg_header(tf_jpeg *enc, const uint8_t **bytes, size_t *n); /* valid as long as the handle (mode 1: see below) */
/* rgb_dev: uint8 [H][W][3] in device memory (tf_comp_image_ptr's, a pixmap's ...).  Queues its kernels on the calling
   thread's stream and waits; header and stream are then copied to `out` (host) and *n_bytes is the file's size.  A file
   larger than `capacity` returns TF_ERR_ARG with *n_bytes the size needed; `out` is then not written at all, and in no
   case is anything written at or beyond out + capacity. */
int tf_jpeg_encode_dev(tf_jpeg *enc, const void *rgb_dev, uint8_t *out, size_t capacity, size_t *n_bytes);
/* The same for an image in host memory: uploaded to a buffer of the handle first. */
int tf_jpeg_encode(tf_jpeg *enc, const uint8_t *rgb_host, uint8_t *out, size_t capacity, size_t *n_bytes);
/* The file of the handle's last encode again, for a caller whose buffer was too small: the intervals are still in
   the handle's staging slots, so only the packing runs again, up to the new capacity.  Same return values;
   TF_ERR_STATE if nothing has been encoded. */
int tf_jpeg_copy_last(tf_jpeg *enc, uint8_t *out, size_t capacity, size_t *n_bytes);
/* The interval restart_mcus = 0 stands for.  No GPU call: a process that only encodes on the host with the same
   settings (transflow_amd/output.py) asks here. */
int tf_jpeg_default_restart_mcus(void);
/* The same encoder with a choice of chroma layout.  `subsampling` is numbered as Pillow's: 0 = 4:4:4 (luma sampling
   1x1: an MCU is 8 x 8 pixels, blocks Y Cb Cr, the chroma samples as converted), 1 = 4:2:2 (2x1: 16 x 8 pixels, blocks
   Y0 Y1 Cb Cr, chroma by libjpeg's h2v1_downsample), 2 = 4:2:0 (2x2: tf_jpeg_create, which equals it) -- Pillow's
   save(quality=q, subsampling=s, restart_marker_blocks=r), byte for byte; of the header only the luma sampling byte of
   SOF0 differs (0x11, 0x21, 0x22).  `restart_mcus` counts MCUs of the layout's own size.  Every other call takes such
   a handle as it takes tf_jpeg_create's, tf_jpeg_set_optimize included (its limit is then 3, 4 or 6 blocks * 64 per
   MCU).  TF_ERR_UNSUPPORTED, with a message, for any other `subsampling`. */
int tf_jpeg_create_sub(tf_jpeg **out, int height, int width, int quality, int restart_mcus, int subsampling);
/* The interval restart_mcus = 0 stands for with that layout: 16, 12, 8 MCUs for 0, 1, 2 -- 48 blocks each.  The first two
   are not tuned as the third is (profiles/jpeg_subsampling_bench.json has them beside half and twice as many).  No GPU
   call.  TF_ERR_UNSUPPORTED for any other `subsampling`. */
int tf_jpeg_default_restart_mcus_for(int subsampling);
/* The Huffman tables of the files.  mode 0 (the default): the Annex K tables, the bytes the files always had.  mode 1:
   the frame's own tables, libjpeg's optimize_coding -- Pillow's save(..., optimize=True), byte for byte: the same pixels
   in a smaller file.  The symbols are counted in a pass of their own, the four tables are made on the device by
   jpeg_gen_optimal_table's rule, and the four DHT segments carry them, so the header's length differs from frame to
   frame.  Makes no GPU call; the mode's buffers are allocated by the first call that needs them.  TF_ERR_ARG for any
   other mode, and for mode 1 on a size of more than 1 000 000 000 coefficients (6 * 64 per MCU).  Changing the mode
   forgets the last file (tf_jpeg_copy_last).
   In mode 1: tf_jpeg_header returns the header of the last encode, valid until the next one, and TF_ERR_STATE before
   any; the encode calls and tf_jpeg_copy_last count with that header's length.  A frame whose tables would need a code
   of more than 32 bits (libjpeg refuses it as JERR_HUFF_CLEN_OVERFLOW) returns TF_ERR_STATE, the message names the
   table, and nothing is written to `out`. */
int tf_jpeg_set_optimize(tf_jpeg *enc, int mode);
/* What the last mode 1 encode built, in the order of the DHT segments (DC luma, AC luma, DC chroma, AC chroma):
   bits[4][16], vals[4][256] (the first sum(bits[t]) of vals[t] are meant, the rest is 0) and, if `counts` is not null,
   the histograms counts[4][257] (entry 256, the reserved symbol, is 1), copied from the device.  TF_ERR_STATE
   if the last call was no such encode. */
int tf_jpeg_last_tables(tf_jpeg *enc, uint8_t *bits, uint8_t *vals, uint32_t *counts);
/* The table stage alone, for tests: the four tables of the histograms counts[4][257] (entry 256 is ignored and taken
   as 1).  *fault: bit t set if table t would need a code of more than 32 bits, and the call returns TF_ERR_STATE.
   TF_ERR_ARG for a histogram whose 256 counts are all zero or sum to more than 1 000 000 000.  Forgets the last file. */
int tf_jpeg_tables_from_counts(tf_jpeg *enc, const uint32_t *counts, uint8_t *bits, uint8_t *vals, uint32_t *fault);

/* ---- PNG of a frame in device memory (transflow/output/frames.py: `-o out/%05d.png`) -----------------------------------
 * 8-bit RGB (colour type 2, no interlace): lossless.  Every row is filtered with the type -- None, Sub, Up, Average,
 * Paeth -- of the smallest sum of min(b, 256 - b); the zlib stream is cut into bands of `band_rows` rows that are coded
 * side by side, each a dynamic-Huffman block over a literal/length code that is a constant of the library
 * (tf_png_code_lengths), with run-length matches (distance 1) only, closed by an empty stored block; one IDAT per band.
 * DESIGN.md section 16 has the rules; any PNG decoder returns the frame's pixels exactly.
 * band_rows: 1 or more (more than the height: one band), 0 = the library's default.  The handle owns its filtered,
 * staging, scan and packed-stream buffers, sized for the worst case at creation. */
typedef struct tf_png tf_png;
int tf_png_create(tf_png **out, int height, int width, int band_rows);
void tf_png_destroy(tf_png *enc);
int tf_png_band_rows(tf_png *enc); /* the rows of a band of this handle */
/* on != 0: the files of the handle's later encodes carry the band index, the ancillary chunk tfBX between IHDR and the
   first IDAT (payload, big-endian: uint8 version 1, uint8 flags 0, uint16 0, uint32 band_rows, uint32 n_bands), which
   tells tf_pngdec that, and how, the IDATs are bands.  Off (the default) the file is what it always was, byte for
   byte.  No GPU call; tf_png_copy_last has nothing to copy until the next encode.  No counterpart in the reference:
   cv2.imwrite (transflow/output/frames.py:31) writes one zlib stream and has no such option. */
int tf_png_set_index(tf_png *enc, int on);
/* The literal/length code of the handle's later encodes.  mode 0 (the default): the library's constant, the bytes the
   files always had.  mode 1: the frame's own -- the tokens of all its bands are counted, the code is built from that
   histogram on the device (the two smallest merged on (weight, order), at most 15 bits, canonical; an unused symbol has
   no code), every coded band carries it in a header of the same 1222 bits, and a band whose coded form would not be
   smaller than its stored form is stored: blocks of at most 65535 bytes behind 00, LEN, NLEN, nothing behind them.
   Everything else about the file is as before and any PNG decoder, tf_pngdec included, reads it.  No GPU call.  No
   counterpart in the reference: cv2.imwrite (transflow/output/frames.py:31) leaves the code to zlib. */
int tf_png_set_code(tf_png *enc, int mode);
/* rgb_dev: uint8 [H][W][3] in device memory.  Queues its kernels on the calling thread's stream and waits; the file is
   then copied to `out` (host) and *n_bytes is its size.  A file larger than `capacity` returns TF_ERR_ARG with *n_bytes
   the size needed; `out` is then not written at all, and in no case is anything written at or beyond out + capacity. */
int tf_png_encode_dev(tf_png *enc, const void *rgb_dev, uint8_t *out, size_t capacity, size_t *n_bytes);
/* The same for an image in host memory: uploaded to a buffer of the handle first. */
int tf_png_encode(tf_png *enc, const uint8_t *rgb_host, uint8_t *out, size_t capacity, size_t *n_bytes);
/* The file of the handle's last encode again, for a caller whose buffer was too small: the bands are still in the
   handle's staging slots, so only the packing runs again, up to the new capacity.  Same return values; TF_ERR_STATE if
   nothing has been encoded. */
int tf_png_copy_last(tf_png *enc, uint8_t *out, size_t capacity, size_t *n_bytes);
/* What the last encode made of the frame, if it ran in mode 1 of tf_png_set_code (TF_ERR_STATE otherwise): the lengths
   of its code's 286 symbols and how often the weights were halved to bring it within 15 bits; the bytes of every band's
   deflate data and whether the band is stored.  *n_bands is the handle's band count; more than `capacity` is TF_ERR_ARG
   and nothing is written.  No GPU call. */
int tf_png_last_code(tf_png *enc, uint8_t *lengths /* [286] */, uint32_t *repairs);
int tf_png_last_bands(tf_png *enc, uint32_t *sizes, uint8_t *stored, size_t capacity, size_t *n_bands);
/* No GPU call in these two.  The rows band_rows = 0 stands for at this size: max(1, ceil(8192 / (3 W + 1))), at most H
   (0 for a size that is none).  The lengths of the literal/length code's 286 symbols. */
int tf_png_default_band_rows(int height, int width);
int tf_png_code_lengths(uint8_t *out /* [286] */);

/* ---- planar YUV of a frame in device memory (transflow/output/ffmpeg.py:32-54: the output that hands raw frames to an
 * encoder) ---------------------------------------------------------------------------------------------------------------
 * The frame in the layout a video encoder takes, made where the frame is: 1.5 to 3 bytes a pixel come down instead of
 * the RGB frame's 3, and no host converts or subsamples.  One tightly packed buffer:
 *   layout 0 yuv444p: Y W*H, U W*H, V W*H;  1 yuv422p: Y, U ceil(W/2)*H, V the same;
 *   2 yuv420p: Y, U ceil(W/2)*ceil(H/2), V the same;  3 nv12: Y, then ceil(H/2) rows of ceil(W/2) pairs U V.
 * matrix 0 bt601, 1 bt709; range 0 tv (Y 16-235, chroma 16-240), 1 pc (0-255).  Integer arithmetic with 16 fractional
 * bits; a chroma sample is the exact mean of its block's unrounded values, rounded once, an odd edge's last column or
 * row repeated (centre-sited: Y4M's C420jpeg).  DESIGN.md section 21 has the rule and the table of coefficients.
 * No counterpart in the reference, whose ffmpeg child converts rgb24 with swscale; these are not swscale's pixels. */
typedef struct tf_yuv tf_yuv;
/* The bytes of a frame in that layout; 0 for a layout or a size that is none.  No GPU call. */
size_t tf_yuv_frame_bytes(int width, int height, int layout);
/* The coefficients as the library builds them: out = the Y, U and V rows, each over (R, G, B); *y_offset 16 or 0.  No
   GPU call: a process that converts on the host with the same arithmetic (transflow_amd/yuv.py host_convert) asks here. */
int tf_yuv_coefficients(int matrix, int range, int32_t out[9], int32_t *y_offset);
/* width, height: 1 to 65535.  The handle owns a device buffer and a page-locked host buffer of one frame. */
int tf_yuv_create(tf_yuv **out, int height, int width, int layout, int matrix, int range);
void tf_yuv_destroy(tf_yuv *h);
/* rgb_dev: uint8 [H][W][3] in device memory, at any address.  Queues the kernel on the calling thread's stream, copies
   the planes to out_host -- directly if that is page-locked memory (tf_host_alloc), else by way of the handle's buffer --
   and waits.  *n_bytes is tf_yuv_frame_bytes; more than `capacity` returns TF_ERR_ARG and nothing is written. */
int tf_yuv_convert_dev(tf_yuv *h, const void *rgb_dev, uint8_t *out_host, size_t capacity, size_t *n_bytes);
/* The same for an image in host memory: uploaded to a buffer of the handle first. */
int tf_yuv_convert(tf_yuv *h, const uint8_t *rgb_host, uint8_t *out_host, size_t capacity, size_t *n_bytes);
/* The planes into the caller's device memory (tf_yuv_frame_bytes bytes at any address, none written outside them):
   queued, not waited for. */
int tf_yuv_convert_to_dev(tf_yuv *h, const void *rgb_dev, void *out_dev);

/* ---- planar YUV frames back to pixels in device memory (transflow_amd/csrc/yuvdec.hip) -------------------------------------
 * The way back: the planes of a Y4M or raw .yuv frame, in the layouts, matrices and ranges above, go up the link and
 * become uint8 [H][W][3] pixels on the device.  With y = Y - 16 (tv) or Y (pc), u = U' - 128, v = V' - 128:
 *   R = clamp((cy y + rv v + 32768) >> 16), G = clamp((cy y + gu u + gv v + 32768) >> 16), B = clamp((cy y + bu u + 32768) >> 16)
 * chroma 0 replicate: U', V' are the sample of the pixel's block;  1 linear: the centre-sited triangle filter (libjpeg's
 * fancy upsampling, neighbour indices clamped at every width).  order 0: R first, 1: B first.  DESIGN.md section 22 has
 * the rule and the table of coefficients.  No counterpart in the reference; these are not swscale's pixels. */
typedef struct tf_yuvdec tf_yuvdec;
/* The coefficients as the library builds them: cy, rv, gu, gv, bu with 16 fractional bits.  No GPU call. */
int tf_yuvdec_coefficients(int matrix, int range, int32_t out[5]);
/* max_width, max_height: 1 to 65535.  The handle owns a page-locked staging buffer and a device buffer of
   tf_yuv_frame_bytes(max_width, max_height, yuv444p) each. */
int tf_yuvdec_create(tf_yuvdec **out, int max_width, int max_height);
void tf_yuvdec_destroy(tf_yuvdec *h);
/* planes_host: the tightly packed frame, nbytes == tf_yuv_frame_bytes(width, height, layout), in any host memory.  Copies it
   to the staging buffer (once that buffer's previous upload has finished), uploads it with one copy on the calling
   thread's stream and queues the kernel; does not wait for the pixels.  out_dev: 3*width*height bytes at any address;
   nothing is written outside them.  TF_ERR_ARG for a bad layout, matrix, range, chroma or order, a size beyond the
   handle, or another nbytes. */
int tf_yuvdec_convert(tf_yuvdec *h, const uint8_t *planes_host, size_t nbytes, int width, int height, int layout, int matrix,
                      int range, int chroma, void *out_dev, int order);
/* The same for planes already in device memory, at any address (a tf_yuv_convert_to_dev result): no copy. */
int tf_yuvdec_convert_dev(tf_yuvdec *h, const void *planes_dev, size_t nbytes, int width, int height, int layout, int matrix,
                          int range, int chroma, void *out_dev, int order);

/* ---- flow archive members deflated on the device (transflow_amd/csrc/flowzip.hip) --------
 * The reference's flow export (transflow/pipeline.py:363-377, 505-506, output/numpy.py, output/zip.py) writes
 * numpy.save(flow) into a deflated zip member.  tf_flowzip makes that member's raw deflate stream -- no zlib header, no
 * Adler-32: what a zip holds -- and the CRC-32 of the uncompressed bytes where the flow is, so that only the member
 * comes down.  The uncompressed stream is S = prefix ‖ data: the `.npy` header (host; a multiple of 64 bytes, as numpy
 * aligns it, at most 4096; 0 for none) and the array's C-order bytes.  S is cut into bands of `band_bytes` that are
 * coded side by side: "the same byte `distance` back" matches only (1 to 64), one literal/length code per member built
 * on the device from the member's own token counts, a band stored where coding it would not make it smaller.
 * DESIGN.md section 17 has the rules; any inflater returns S.
 * band_bytes: a multiple of 64, 0 = the library's default.  The handle owns its count, scan and stream buffers, sized
 * at creation for streams of up to max_stream_bytes (at most 2^31): the stream is never longer than
 * N + 5 per stored block of 65535 bytes + 5. */
typedef struct tf_flowzip tf_flowzip;
int tf_flowzip_create(tf_flowzip **out, size_t max_stream_bytes, int band_bytes);
void tf_flowzip_destroy(tf_flowzip *enc);
int tf_flowzip_band_bytes(tf_flowzip *enc); /* the bytes of a band of this handle */
int tf_flowzip_default_band_bytes(void);    /* what band_bytes = 0 stands for; no GPU call */
/* data_dev: data_bytes in device memory, read where they are.  Queues its kernels on the calling thread's stream and
   waits; the stream is then copied to `out` (host), *n_bytes is its size and *crc32 the CRC-32 of S.  A stream larger
   than `capacity` returns TF_ERR_ARG with *n_bytes the size needed; `out` is then not written at all, and in no case is
   anything written at or beyond out + capacity. */
int tf_flowzip_encode_dev(tf_flowzip *enc, const uint8_t *prefix_host, size_t prefix_len, const void *data_dev, size_t data_bytes,
                          int distance, uint8_t *out, size_t capacity, size_t *n_bytes, uint32_t *crc32);
/* The same for data in host memory: uploaded to a buffer of the handle first. */
int tf_flowzip_encode(tf_flowzip *enc, const uint8_t *prefix_host, size_t prefix_len, const void *data_host, size_t data_bytes,
                      int distance, uint8_t *out, size_t capacity, size_t *n_bytes, uint32_t *crc32);
/* The stream of the handle's last encode again, for a caller whose buffer was too small: it is still in the handle, no
   kernel runs.  Same return values; TF_ERR_STATE if nothing has been encoded. */
int tf_flowzip_copy_last(tf_flowzip *enc, uint8_t *out, size_t capacity, size_t *n_bytes);
/* The lengths of the last member's literal/length code, 286 symbols (0: unused). */
int tf_flowzip_last_lengths(tf_flowzip *enc, uint8_t *out /* [286] */);
/* The compressed bytes of each band of the handle's last encode, in stream order (they sum, with the five bytes of the
   final block, to the stream's size): what a reader needs to inflate the bands side by side.  Read from the handle's
   size words; no kernel runs.  The handle keeps no band count: it is inferred as the number of leading size words that sum
   to the stream's size without the final block (every band has at least six bytes).  *n_bands is the band count; TF_ERR_STATE before the first encode, TF_ERR_ARG (with
   *n_bands set) if `capacity` is smaller. */
int tf_flowzip_last_band_sizes(tf_flowzip *enc, uint32_t *out, size_t capacity, size_t *n_bands);
/* numpy.round(flow).astype(int) of n_values float32 (wide = 0) or float64 (wide = 1) values in device memory: rounded
   half to even in the input's type, then converted; a value that does not fit, or a NaN, gives 0x8000000000000000 (what
   numpy gives on x86-64).  out_dev: n_values int64.  Queued on the calling thread's stream; does not wait. */
int tf_flow_round_i64_dev(const void *flow_dev, size_t n_values, int wide, void *out_dev);

/* ---- flow archive members inflated on the device (transflow_amd/csrc/flowunzip.hip) --------
 * The inverse of tf_flowzip for a member whose bands' compressed sizes are known (the archive's band index, DESIGN.md
 * section 18): band b is bytes [offset_b, offset_b + size_b) of the member's raw deflate stream and must inflate, on its
 * own, to exactly bytes [b * band_bytes, min(usize, (b + 1) * band_bytes)) of S = the `.npy` header ‖ the array.  A band
 * is any sequence of RFC 1951 blocks with BFINAL 0 -- stored, fixed, dynamic -- whose matches stay inside the band's own
 * output and whose last block ends on the range's last bit: tf_flowzip's bands and zlib's Z_FULL_FLUSH bands are such.
 * Anything else is rejected per band with no access outside the band's ranges.  What follows the last band (the final
 * block) is not decoded: the caller checks it.
 * Bytes of S below `split` (a multiple of 64, at most 4096, 0 for none) come down to head_out_host; bytes from `split`
 * on go to data + (index - split).  *crc32 is the CRC-32 of S, computed on the device. */
typedef struct tf_flowunzip tf_flowunzip;
int tf_flowunzip_create(tf_flowunzip **out, size_t max_stream_bytes, size_t max_bands);
void tf_flowunzip_destroy(tf_flowunzip *h);
/* stream_host: the compressed bytes (page-locked memory is copied at the link's rate); band_sizes_host: n_bands sizes.
   data_dev: usize - split bytes of device memory, 4-byte aligned.  Queues on the calling thread's stream and waits.
   TF_ERR_ARG (nothing is launched): split or band_bytes no multiple of 64 or out of range, sizes that sum past
   stream_bytes, n_bands != ceil(usize / band_bytes), more than the handle was made for.  TF_ERR_STATE: a band was
   rejected; *bad_band is the first such (0xFFFFFFFF otherwise) and the destination's contents are undefined.
   A band's decoding time is bounded by its compressed bits, not by its output: every dynamic block costs three table
   constructions in one lane, however little it holds.  A caller with untrusted input bounds the bands' sizes first
   (transflow_amd/archive.py: at most 2 * band_bytes + 1024 bytes a band, band_bytes at most 1 MiB). */
int tf_flowunzip_decode_dev(tf_flowunzip *h, const uint8_t *stream_host, size_t stream_bytes, const uint32_t *band_sizes_host,
                            size_t n_bands, size_t band_bytes, size_t usize, size_t split, uint8_t *head_out_host, void *data_dev,
                            uint32_t *crc32, uint32_t *bad_band);
/* The same into host memory (through a buffer of the handle). */
int tf_flowunzip_decode(tf_flowunzip *h, const uint8_t *stream_host, size_t stream_bytes, const uint32_t *band_sizes_host,
                        size_t n_bands, size_t band_bytes, size_t usize, size_t split, uint8_t *head_out_host, void *data_host,
                        uint32_t *crc32, uint32_t *bad_band);
/* astype(float32) of n_values int64 in device memory: to nearest, ties to even, as numpy converts.  Queued on the
   calling thread's stream; does not wait. */
int tf_flow_i64_to_f32_dev(const void *src_dev, size_t n_values, void *dst_dev);

/* ---- baseline JPEG decoded on the device (transflow_amd/csrc/jpegdec.hip) ----------------
 * The inverse of tf_jpeg for more than its own files: SOF0, 8-bit, one scan that interleaves all components, three
 * components (luma sampled 2x2, 2x1 or 1x1, chroma 1x1) or one, 8-bit DQT, any valid DHT, any restart interval or
 * none.  The pixels are libjpeg's (islow IDCT, fancy upsampling), bit for bit.  The compressed bytes go up; the restart
 * intervals are decoded side by side, one wave each, so a file without DRI is decoded by one wave.
 * Every other file is rejected whole, with a reason (tf_jpegdec_reject_name; the enum is jpegdec_common.h's Reject).
 * A rejection is a status, not an error: the call returns TF_OK and *reject != 0.  Nothing is then promised about
 * the output buffer except that nothing outside it was written. */
typedef struct tf_jpegdec tf_jpegdec;
typedef struct { int width, height, components, h_samp, v_samp, restart_mcus, intervals; uint32_t reject; } tf_jpegdec_info;
/* The header alone (host only, no GPU call): the geometry, or why the header is rejected. */
int tf_jpegdec_probe(const uint8_t *file, size_t n, tf_jpegdec_info *info);
int tf_jpegdec_create(tf_jpegdec **out, int max_width, int max_height, size_t max_file_bytes);
void tf_jpegdec_destroy(tf_jpegdec *dec);
/* order: 0 RGB, 1 BGR.  out_dev: uint8 [height][width][3].  Queues on the calling thread's stream and waits for the
   status.  Returns TF_OK with *reject != 0 for a file the device does not take; TF_ERR_ARG for a frame larger than
   the handle was made for or a NULL pointer. */
int tf_jpegdec_decode_dev(tf_jpegdec *dec, const uint8_t *file, size_t n, void *out_dev, int order, uint32_t *reject);
/* The same into host memory (through a buffer of the handle); out_host is written only when *reject == 0. */
int tf_jpegdec_decode(tf_jpegdec *dec, const uint8_t *file, size_t n, uint8_t *out_host, int order, uint32_t *reject);
const char *tf_jpegdec_reject_name(uint32_t reject);
/* How a file WITHOUT a restart interval is entropy-decoded (files with DRI go one wave per interval in either mode):
   0 (the default): as one interval, by one wave.  1: the scan is cut into subsequences of bytes, one lane each; every
   lane decodes from a guessed state and hands its exit state to its neighbour until nothing changes (a Huffman decoder
   started at a wrong bit finds the right code boundaries by itself after a while), then the blocks' numbers and DC
   predictions are summed up and every lane decodes once more into place.  Same pixels, same verdicts.  The path's
   buffers (sized by the handle's limits) are allocated by the first decode that takes it. */
int tf_jpegdec_set_scan_mode(tf_jpegdec *dec, int mode);
/* Of the last decode that took the parallel path: subsequences, work-groups, launches of the synchronisation kernel
   (at most work-groups + 1), the largest number of rounds any work-group made in a launch (at most its lanes). */
int tf_jpegdec_par_stats(tf_jpegdec *dec, uint32_t out[4]);
/* For tests: per subsequence of that decode, 8 words into rows[capacity][8] -- the entry state's bit position (low word,
   high word; a bit index into the scan, stuffed bytes included), block within the MCU and coefficient index k (0: a DC
   code comes next), the number of the first block that begins in the subsequence and the three components' DC
   predictions there (modulo 2^32).  *n_subs: the subsequences; TF_ERR_ARG when capacity is less. */
int tf_jpegdec_par_entries(tf_jpegdec *dec, uint32_t *rows, size_t capacity, uint32_t *n_subs);

/* ---- banded PNG frames decoded on the device (transflow_amd/csrc/pngdec.hip) --------------
 * The inverse of tf_png for the files it writes with tf_png_set_index, and for any file of that shape: 8-bit RGB, colour
 * type 2, not interlaced; IHDR, tfBX, an IDAT with a two-byte zlib header, one IDAT per band of band_rows rows, an
 * IDAT with an empty final block and the Adler-32, IEND.  A band is any sequence of non-final deflate blocks that ends
 * on a byte and whose matches stay inside the band's own output (tf_png's bands, zlib's Z_FULL_FLUSH bands).  It stands
 * where the reference decodes a frame of an image sequence on the host and the pixels go up: cv2.VideoCapture.read()
 * in transflow/pixmap/cv.py:54 (a moving pixmap) and transflow/flow/sources/cv.py:451, 461 (the video a flow is
 * computed from).  The compressed file goes up; chunk CRCs, inflate (one wave per band), Adler-32 and the row filters
 * are done on the device and the pixels are written once, where the caller wants them.
 * A reject word is reason | where << 8: `where` is the chunk (chunk_crc; IHDR is chunk 0), the row (filter_type) or the
 * band (band_*), else 0; tf_pngdec_reject_name names the reason (pngdec_common.h's Reject).
 * A band's decoding time is bounded by its compressed bits, as tf_flowunzip's: a direct caller with untrusted files sets
 * a bound on the bands first, as transflow_amd/pngdec.py does (a band of at most 1 MiB of output and of at most
 * 2 * that + 1024 compressed bytes; other files are decoded on the host). */
typedef struct tf_pngdec tf_pngdec;
typedef struct {
    int width, height, band_rows, n_bands;
    int indexed;             /* 1: a file for the device */
    int why_not;             /* a well-formed file that is not: 1 no index, 2 not 8-bit RGB, 3 interlaced, 4 an index of an unknown version */
    uint32_t reject;         /* a malformed file: the reject word (then neither of the above) */
    uint32_t max_band_bytes; /* the largest band's compressed bytes */
    uint32_t *band_offsets, *band_sizes; /* in: arrays of band_capacity entries (or NULL, 0); out: where each band's
                                            compressed bytes begin in the file, and how many they are */
    size_t band_capacity;
} tf_pngdec_info;
/* The chunks alone, walked on the host (no GPU call; CRCs are not looked at): every length is checked against the file
   before it is used.  Always TF_OK for non-null arguments; info->reject, info->indexed and info->why_not say which of
   the three a file is: rejected, for the device, or a PNG of another kind (which is no error).
   Replaces the container probing of cv2.VideoCapture(path) (transflow/pixmap/cv.py:34, flow/sources/cv.py:421). */
int tf_pngdec_probe(const uint8_t *file, size_t n, tf_pngdec_info *info);
/* Frames of up to max_width x max_height (each at most 2^24 - 1, together at most 2^31 filtered bytes) in files of up to
   max_file_bytes; the staging buffer (page-locked) and every device buffer are allocated here.  Stands where the
   reference opens its capture: cv2.VideoCapture(path) (transflow/pixmap/cv.py:34, transflow/flow/sources/cv.py:421). */
int tf_pngdec_create(tf_pngdec **out, int max_width, int max_height, size_t max_file_bytes);
/* Replaces capture.release() (transflow/pixmap/cv.py:66, transflow/flow/sources/cv.py:524). */
void tf_pngdec_destroy(tf_pngdec *dec);
/* file_host: the file; pix_dev: uint8 [height][width][3] in device memory, RGB, or BGR with bgr = 1 (what a flow source
   wants); nothing outside these bytes is written.  Queues on the calling thread's stream and waits for the status.
   TF_ERR_ARG (nothing is launched): a NULL pointer, a file larger than the handle's, a file that is not for the device.
   TF_ERR_STATE with *reject set: a file the walk rejects (a frame beyond the handle's size is `size`), a chunk whose
   CRC differs, a band that is no valid band, a filter type above 4, an Adler-32 that differs; the pixels are then
   undefined.  Replaces capture.read() (transflow/pixmap/cv.py:54, transflow/flow/sources/cv.py:451, 461). */
int tf_pngdec_decode_dev(tf_pngdec *dec, const uint8_t *file_host, size_t n, void *pix_dev, int bgr, uint32_t *reject);
/* The same into host memory (through a buffer of the handle); pix_host is written only when the file is accepted. */
int tf_pngdec_decode(tf_pngdec *dec, const uint8_t *file_host, size_t n, uint8_t *pix_host, int bgr, uint32_t *reject);
/* The name of a reject word's reason ("ok" for 0, "unknown" for a number that is none).  No counterpart in the
   reference, whose capture.read() says only success or not (transflow/pixmap/cv.py:54-55). */
const char *tf_pngdec_reject_name(uint32_t reject);

/* ---- numpy's legacy random stream on the device (MT19937; numpy.random.random, reference.py:59) --------------------
 * A handle draws the stream RandomState draws, bit for bit, into device memory: fields of n doubles, each double from two
 * consecutive tempered 32-bit words a, b as ((a >> 5) * 2^26 + (b >> 6)) / 2^53.  It works on word positions: the raw
 * words obey x[k + 624] = x[k + 397] ^ twist(x[k], x[k + 1]) at every k, so any 624 consecutive raw words are a state.
 * A field's 2 n words are cut into segments, one wave each; every segment's start state for the next field is t^(2 n)
 * mod the characteristic polynomial applied to its start state for this one.  A new state or another n costs a one-time
 * bootstrap (one wave walks the field's span) and, with more than one segment, that polynomial (host, milliseconds). */
typedef struct tf_mt tf_mt;
int tf_mt_create(tf_mt **out);      /* the state of seed 5489 until tf_mt_set_state */
void tf_mt_destroy(tf_mt *mt);
/* numpy's state tuple: key[624] and pos, 0..624 (odd ones included; the first words come from the current block). */
int tf_mt_set_state(tf_mt *mt, const uint32_t *key /*[624]*/, int pos);
/* An equivalent state of the stream's position: the next 624 raw words and *pos = 0.  Waits for the draws queued. */
int tf_mt_get_state(tf_mt *mt, uint32_t *key /*[624]*/, int *pos);
/* The next n doubles of the stream (1 <= n <= 2^30) into out_dev (8-byte aligned), queued on the caller's stream. */
int tf_mt_random_sample_dev(tf_mt *mt, void *out_dev, size_t n);
/* The plan of the last draw: segments, words of a segment, milliseconds of the last bootstrap's walk (any may be NULL). */
int tf_mt_info(tf_mt *mt, int *segments, int *segment_words, float *bootstrap_ms);
/* Host-only entry points, callable without a GPU.  Polynomials over GF(2): TF_MT_POLY_WORDS 64-bit words, bit i of word
   i / 64 the coefficient of t^i.
   _charpoly: the characteristic polynomial phi by Berlekamp-Massey over the generator's own output (its degree, 19937,
   in *degree; the coefficients below t^19937 in coeff_words -- the leading one is implied).
   _jump_poly: t^J mod phi.  _apply: out[j] = XOR over poly's set coefficients i of x[i + j], j < 624, x the raw stream
   whose first 624 words are key (word 0 taken as the recurrence would have produced it: only its top bit is state):
   with poly = t^J mod phi, J >= 1, that is x[J .. J + 623].  _random_sample: RandomState.random_sample(n) from numpy's
   (key, pos), in numpy's own block-by-block form. */
#define TF_MT_POLY_WORDS 312
int tf_mt_stage_charpoly(int *degree, uint64_t *coeff_words /*[TF_MT_POLY_WORDS]*/);
int tf_mt_stage_jump_poly(uint64_t J, uint64_t *out /*[TF_MT_POLY_WORDS]*/);
int tf_mt_stage_apply(const uint64_t *poly, const uint32_t *key, uint32_t *out /*[624]*/);
int tf_mt_stage_random_sample(const uint32_t *key, int pos, size_t n, double *out);

/* ---- batch-of-frames mode over the GPUs of one node ----------------------
 * With flags == 0 every Farnebäck pair is independent (transflow/flow/sources/cv.py:478-490: the
 * `flow=` argument is an output buffer only), so ranks take contiguous ranges of pairs and the path
 * needs no data-path collective.  What is exchanged, through RCCL over xGMI on the library stream:
 * the shared inputs once (broadcast: the pixmap every rank's compositor gathers from,
 * compositor/layers/reference.py:93-105, and the reset mask, reference.py:44) and finished frames to
 * one rank (gather: what Pipeline hands to its output, pipeline.py:518).  One process per GPU; the
 * communicator binds to the device tf_init selected.  librccl is loaded on the first tf_batch_* call.
 * The 128-byte id is made on rank 0 and carried to the other ranks by the host (file or socket). */
#define TF_BATCH_ID_BYTES 128
typedef struct tf_batch tf_batch;
int tf_batch_unique_id(uint8_t *id /*[TF_BATCH_ID_BYTES]*/);
int tf_batch_init(tf_batch **out, int rank, int world, const uint8_t *id);
void tf_batch_destroy(tf_batch *batch);
int tf_batch_info(tf_batch *batch, int *rank, int *world, int *rccl_version); /* any pointer may be NULL */
/* In place: root's `bytes` at dev reach every rank's dev. */
int tf_batch_broadcast(tf_batch *batch, void *dev, size_t bytes, int root);
/* Rank r's send_bytes land on root at recv_dev + sum(recv_bytes[0..r)); recv_bytes NULL = every rank
   sends send_bytes.  recv_dev / recv_bytes are read on root only.  Point-to-point sends into the root
   (all its inbound links at once), not a ring. */
int tf_batch_gather(tf_batch *batch, const void *send_dev, size_t send_bytes, void *recv_dev, const size_t *recv_bytes,
                    int root);
/* The gather with explicit places: rank r's send_bytes land on root at recv_dev + recv_offsets[r] (ranges inside
   recv_capacity, not overlapping; a rank with nothing to send passes 0).  "Flows to root" (mode F): the
   flows of a rank's pass land at the clip position of the pass's first pair, and the root's one compositor consumes
   the clip's flows in order, as the reference's one compositor does (transflow/pipeline.py:565 hands every flow of
   the clip to Compositor.update in turn; compositor/layers/movement.py:51-52 is the recurrence that makes the
   order matter). */
int tf_batch_gather_at(tf_batch *batch, const void *send_dev, size_t send_bytes, void *recv_dev, const size_t *recv_bytes,
                       const size_t *recv_offsets, size_t recv_capacity, int root);
/* The same gather beside the library stream's next work (transflow/pipeline.py:518 takes one frame at a time; a batch of
   finished frames need not hold up the next batch): _begin starts it, on a stream of the communicator's own, once the
   library stream has reached the point of the call; _end makes the library stream wait for it on the device.  One at
   a time; call _end before the send buffer is written again. */
int tf_batch_gather_begin(tf_batch *batch, const void *send_dev, size_t send_bytes, void *recv_dev, const size_t *recv_bytes,
                          int root);
int tf_batch_gather_end(tf_batch *batch);
/* values[n] (host) := sum (op 0) or max (op 1) over ranks; n <= 63.  Waits for the library stream on
   every rank: with n = 0 it is the barrier a timed region is bracketed with. */
int tf_batch_reduce(tf_batch *batch, double *values, int n, int op);

#ifdef __cplusplus
}
#endif
#endif /* TFHIP_H */
