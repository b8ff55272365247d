/*
 * higsfa.h — C ABI of the MI355X-native HiGSFA inference path.
 *
 * Drop-in boundary for PyFaceAnalysis' hot call
 *
 *     sl = networks[num_network].execute(subimages_arr, benchmark=benchmark)
 *                                      (reference: FaceDetectUpdated.py:699;
 *                                       also face_analysis.py:1064 and :1257)
 *
 * The reference has no native code and no FFI; these entry points are what a
 * ctypes/cffi binding for that one call needs: load a flow description, run batches of
 * flattened sub-images through it on one GPU, read results and per-stage timings back.
 * Plain C types only.  All functions return 0 (HG_OK) on success or a negative hg_status;
 * hg_last_error() returns a thread-local message for the last failure on the calling thread.
 *
 * Threading: one hg_flow may be used by one thread at a time; different flows are
 * independent.  The library keeps no global mutable state besides the last-error string and the two lane streams per device
 * (hg_lane_stream_id), which are created once under a lock and never changed.
 * There is NO CPU execution path: without a usable HIP device hg_flow_to_device /
 * hg_flow_execute* fail with HG_ERR_DEVICE.
 */
#ifndef HIGSFA_H
#define HIGSFA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HG_VERSION 100 /* 0.1.0 */

typedef struct hg_flow hg_flow;

/* Element types accepted for the sub-image matrix / produced for the feature matrix.
 * The reference passes float64 arrays holding integer pixel values 0..255
 * (images_asarray, face_analysis.py:786) and receives float64 (MDP node dtype). */
enum hg_dtype { HG_U8 = 0, HG_F32 = 1, HG_F64 = 2 };

enum hg_status {
    HG_OK = 0,
    HG_ERR_ARG = -1,      /* null pointer, bad dtype, bad leading dimension, ...            */
    HG_ERR_FORMAT = -2,   /* malformed / truncated / unsupported blob                        */
    HG_ERR_DIM = -3,      /* input_dim / output_dim mismatch (MDP raises on these too)        */
    HG_ERR_DEVICE = -4,   /* no HIP device, HIP call failed, flow not on a device; also: a persistent kernel of an
                           * earlier call on this flow reported a failed internal hand-off (its features are invalid) */
    HG_ERR_NOMEM = -5,
    HG_ERR_STATE = -6     /* call made in the wrong state (e.g. timings without profiling)    */
};

/* Which execution plan the loader chose for a flow. */
enum hg_plan_kind {
    HG_PLAN_GENERIC = 0,  /* step-by-step kernels on row-major activations (any flow)         */
    HG_PLAN_FUSED = 1     /* per-layer fused gather+affine+expansion+affine MFMA kernels       */
};

typedef struct hg_info {
    int64_t input_dim;        /* columns of x  (mdp Flow: flow[0].input_dim)                   */
    int64_t output_dim;       /* columns of y  (flow[-1].output_dim)                           */
    int32_t n_top_nodes;      /* len(flow) — top-level nodes as the reference's flow has them  */
    int32_t plan_kind;        /* enum hg_plan_kind                                             */
    int32_t n_stages;         /* kernels (fused) or steps (generic) launched per execute       */
    int32_t device;           /* HIP device ordinal, -1 while host-only                        */
    int64_t weight_bytes;     /* device bytes held by weights/descriptors                      */
    int64_t flops_per_row;    /* algorithmic FLOPs per sub-image: sum 2*in*out over affines    */
    int64_t padded_flops_per_row; /* FLOPs the fused MFMA tiling issues per row, every layer with its own first affine (hoisted links issue fewer: hg_flow_describe) */
    int64_t workspace_bytes;  /* device bytes currently reserved for activations              */
} hg_info;

int hg_version(void);
const char* hg_last_error(void);

/* Number of visible HIP devices (0 and HG_OK when there are none / no driver). */
int hg_device_count(int* count);

/* Parse a flow blob ("HGSFAFL1", see pyfaceanalysis_amd/blob.py) and build the execution
 * plan on the host.  Replaces: cache_obj.load_obj_from_cache (pickle) in
 * face_analysis.py:457.  Touches no GPU.  `flags`: bit0 = force the generic plan. */
int hg_flow_load(const void* blob, size_t nbytes, int flags, hg_flow** out);
void hg_flow_free(hg_flow* f);

int hg_flow_info(const hg_flow* f, hg_info* info);

/* Human-readable plan listing (counterpart of more_nodes.describe_flow,
 * FaceDetectUpdated.py:193).  Writes at most cap-1 chars + NUL; returns needed length in
 * *needed when non-null. */
int hg_flow_describe(const hg_flow* f, char* buf, size_t cap, size_t* needed);

/* Upload weights/descriptors to HIP device `device` (one device per flow handle). */
int hg_flow_to_device(hg_flow* f, int device);

/* Pre-size the activation workspace for batches of up to `max_rows` rows so that
 * hg_flow_execute_device performs no allocation. */
int hg_flow_reserve(hg_flow* f, int64_t max_rows);

/* y[n, 0:y_cols] = flow(x[n, :]) with HOST buffers (the ndarray-in / ndarray-out call of
 * FaceDetectUpdated.py:699).  x: n rows of input_dim elements, row stride ldx elements;
 * y: n rows, the first y_cols (<= output_dim) columns, row stride ldy elements.  The caller
 * usually wants only the first classifier.input_dim columns (FaceDetectUpdated.py:709,719).
 * n == 0 is valid and a no-op (reference guards len(subimages_arr) > 0 at :694).
 * Synchronous: returns after y is complete.  A pool of host threads on the memory node of the rows packs them while the
 * device works on earlier rows (passes of a few hundred rows, sized by a planner): straight into device memory on large-BAR
 * devices, through a pinned ring and two copy queues otherwise; float32 / float64 rows whose values are all integers 0..255 —
 * what images_asarray produces (face_analysis.py:786) — cross PCIe as uint8, which changes no output bit; from the first
 * row that holds anything else the rest of the call travels in the caller's own type. */
int hg_flow_execute(hg_flow* f, const void* x, int x_dtype, int64_t n, int64_t ldx,
                    void* y, int y_dtype, int64_t y_cols, int64_t ldy);

/* The same call over several devices of this process (sub-images are independent, so the batch is
 * cut into n_devices contiguous row blocks of ceil(n / n_devices) rows; block r runs on devices[r] with replicated
 * weights, its own streams and staging buffers, driven by its own host thread; every block's features land in the
 * caller's y at the block's rows — with host buffers that IS the gather, no peer copy or collective is needed).
 * devices == NULL means 0 .. n_devices-1; a device may be listed more than once (each entry is a replica).
 * Replicas are created on first use and kept in the handle; hg_flow_to_device is not required.
 * Multi-process callers (one rank per GPU, RCCL all-gather of device-resident features) use
 * hg_flow_execute_device per rank instead: pyfaceanalysis_amd/sharded.py. */
int hg_flow_execute_sharded(hg_flow* f, const void* x, int x_dtype, int64_t n, int64_t ldx,
                            void* y, int y_dtype, int64_t y_cols, int64_t ldy,
                            const int* devices, int n_devices);

/* Same with DEVICE buffers on the flow's device, enqueued on `stream` (hipStream_t, may be
 * null = default stream); returns without synchronising. */
int hg_flow_execute_device(hg_flow* f, const void* x_dev, int x_dtype, int64_t n, int64_t ldx,
                           void* y_dev, int y_dtype, int64_t y_cols, int64_t ldy, void* stream);

/* --- Step lanes: two steps in flight through ONE flow handle -----------------------------------------------
 * A step's eight launches ramp up and tail off; two independent batches that share the chip fill each other's ramps.  A lane is
 * one copy of everything a call WRITES (activation workspace, tile-queue counters, error word) over the handle's one copy of
 * what it only reads (weights, tables, plans), plus a stream of its own.  hg_flow_set_lanes(f, n), n = 1 or 2, after
 * hg_flow_to_device: HG_ERR_STATE (and the handle stays serial) where the plan keeps one set of state — the generic plan does.
 * It first waits for whatever the handle has in flight on a lane.  hg_flow_reserve sizes every lane; workspace_bytes in hg_info is
 * their sum.  The two lane streams exist once per device and process and are shared by all flows on the device (which hardware
 * queue a stream lands on depends on how many the process created before it); hg_lane_stream_id returns the stream of (device,
 * lane) as an integer (it is a hipStream_t), creating the pair on first use.
 *
 * hg_flow_step_lane_device(f, lane, x, ..., y, ..., ready_stream): records the lane's "ready" event on ready_stream and makes the
 * lane's stream wait for it — so everything enqueued on ready_stream so far (the producer of x, the last reader of y) precedes the
 * step — then enqueues exactly the launches of hg_flow_execute_device on the lane's stream with the lane's state, then records the
 * lane's "done" event there.  Returns without synchronising; the features are NOT ordered on ready_stream: wait for the done event
 * (hg_flow_lane_done_event: a hipEvent_t owned by the handle, device scope like hg_event_create's, re-recorded by the lane's next
 * step) or call hg_flow_lane_join(f, lane, stream), which makes `stream` wait for the lane's last step (a no-op before the first).
 * A lane whose workspace must grow first waits for its own last step (and freeing the old buffers drains the device).  Never profiled.
 * hg_flow_execute_device keeps its contract — lane 0's state, the caller's stream, strictly ordered there; it waits for a lane-0
 * step that is still in flight.  A lane-0 step that follows it is ordered behind it only through ready_stream.
 * hg_flow_check_errors reads every lane's error word (meaningful after a synchronisation); hg_flow_free first waits for every
 * lane.  One thread per handle, as for every other call. */
int hg_flow_set_lanes(hg_flow* f, int n);
int hg_flow_lanes(const hg_flow* f, int* n);
int hg_flow_step_lane_device(hg_flow* f, int lane, const void* x_dev, int x_dtype, int64_t n, int64_t ldx,
                             void* y_dev, int y_dtype, int64_t y_cols, int64_t ldy, void* ready_stream);
int hg_flow_lane_done_event(hg_flow* f, int lane, void** ev);
int hg_flow_lane_join(hg_flow* f, int lane, void* stream);
int hg_flow_check_errors(hg_flow* f);
int hg_lane_stream_id(int device, int lane, uint64_t* id);

/* Device-scope events for callers that overlap a collective with the next batch (pyfaceanalysis_amd/sharded.py: the RCCL
 * all-gather of the features on a side stream, ordered against the kernels in both directions).  Created with
 * hipEventDisableTiming | hipEventDisableSystemFence: recording one does not write the caches back to system scope the way
 * a default event does (measured on an MI355X: 13 us between two launches of the stream it is recorded on, against < 2).
 * They order device work only — nothing the host reads may depend on them.  `ev` is an opaque handle (hipEvent_t),
 * streams are hipStream_t of the calling thread's current device. */
int hg_event_create(void** ev);
/* The same on a stated device, whatever the calling thread's current device is (which it leaves unchanged), and with the
 * choice of scope: device_scope 0 creates an ordinary (hipEventDisableTiming) event whose record also publishes to system
 * scope — what pyfaceanalysis_amd/sharded.py uses for the hand-off that carries DATA to the collective unless a run on more
 * than one GPU has verified the device-scope form (bench.py does that before it times anything). */
int hg_event_create_on(void** ev, int device, int device_scope);
void hg_event_destroy(void* ev);
int hg_event_record(void* ev, void* stream);
int hg_stream_wait_event(void* stream, void* ev);
/* 1 when everything the event was last recorded behind has completed, 0 when not yet (never blocks); < 0: hg_status.
 * Lets the host skip a wait that would only put a barrier packet in front of the next launch (measured: 4.5 us). */
int hg_event_query(void* ev);
/* Blocks the calling thread until everything the event was last recorded behind has completed (the host learns THAT the work is
 * done; what it then reads goes through a copy or a kernel of its own, as after any device-scope event). */
int hg_event_synchronize(void* ev);

/* How the last hg_flow_execute of this handle moved the caller's rows (FaceDetectUpdated.py:699 hands over a host ndarray,
 * face_analysis.py:786): *transport = 1 — packer threads stored the wire rows straight into device memory, which is done only
 * where the device reports a large BAR AND hsa_amd_pointer_info confirms every input buffer host-mapped at its device address;
 * 0 — pinned ring + copy queues (HIGSFA_HOST_DIRECT=0, or any other answer of the probe); -1 — no such call yet. */
int hg_flow_host_transport(const hg_flow* f, int* transport);
/* What bounds that call on THIS box, measured in the caller's process (bench.py puts them beside the host-path figures):
 * hg_host_pack_probe — the library's packer threads alone over the caller's array (same pool, placement and routines as
 * hg_flow_execute; destinations stay in cache): the rate at which the host can read and narrow / copy these rows;
 * hg_host_store_probe — the packers storing `bytes` from host memory straight into device memory (*direct = 0 and no time where
 * hg_flow_execute would not do that either); hg_host_dma_probe — one pinned-memory copy of `bytes` through the copy engine.
 * best_seconds: best of `reps` rounds after one untimed round. */
int hg_host_pack_probe(const void* x, int x_dtype, int64_t n, int64_t ldx, int64_t in_dim, int reps, double* best_seconds);
int hg_host_store_probe(int device, size_t bytes, int reps, double* best_seconds, int* direct);
int hg_host_dma_probe(int device, size_t bytes, int reps, double* best_seconds);
/* Per-stage timing (the `benchmark=` kwarg of the reference call; benchmarking.py:39-58).
 * When enabled every stage launch is bracketed by hipEvents on the execution stream. */
int hg_flow_set_profiling(hg_flow* f, int enabled);
/* After a profiled execute has completed: accumulated ms and launch count per stage since
 * the last reset; `cap` entries at most; *n_stages receives the stage count. */
int hg_flow_stage_times(hg_flow* f, double* total_ms, int64_t* launches, int cap, int* n_stages);
int hg_flow_stage_name(const hg_flow* f, int stage, char* buf, size_t cap);
int hg_flow_reset_profile(hg_flow* f);

/* --- Gaussian-classifier soft-label regression -------------------------
 * The step right after the hot call: classifiers[k].regression(sl[:, 0:d], avg_labels)
 * (FaceDetectUpdated.py:709-719).  Parameters as stored in the SavedClassifiers pickles:
 * means (K,d), inv_covs (K,d,d), sqrt_det_covs (K), priors p (K), avg_labels (K); float64.
 * out_reg[n] = sum_c post_c(x_n) avg_labels[c]; out_std (optional) the posterior std. */
typedef struct hg_gauss hg_gauss;
int hg_gauss_create(int32_t n_classes, int32_t dim, const double* means, const double* inv_covs,
                    const double* sqrt_det_covs, const double* priors, const double* avg_labels,
                    int device, hg_gauss** out);
void hg_gauss_free(hg_gauss* g);
/* x_dev: (n, >=dim) device matrix of dtype x_dtype (F32/F64), row stride ldx; outputs are
 * device float64 arrays of n elements (out_std may be null).  Enqueued on `stream`. */
int hg_gauss_regression_device(hg_gauss* g, const void* x_dev, int x_dtype, int64_t n, int64_t ldx,
                               double* out_reg_dev, double* out_std_dev, void* stream);
/* m <= 4 classifiers on the SAME feature rows in one launch — a cascade stage that owns a network and the stages behind it whose
 * network is None reuse one sl (FaceDetectUpdated.py:678-682, :704-706; Pipelines/Pipeline_experimental.txt:8-19): regressions of
 * classifier s go to out_reg_dev[s * out_stride + row].  Same bits as m calls of hg_gauss_regression_device. */
int hg_gauss_regression_multi_device(hg_gauss* const* gs, int m, const void* x_dev, int x_dtype, int64_t n, int64_t ldx,
                                     double* out_reg_dev, int64_t out_stride, void* stream);
/* Host-buffer convenience wrapper (synchronous). */
int hg_gauss_regression(hg_gauss* g, const void* x, int x_dtype, int64_t n, int64_t ldx,
                        double* out_reg, double* out_std);

/* --- On-device sub-image extraction ---------------------------------------
 * The producer of the hot call's input: load_network_subimages -> extract_subimages_rotate
 * (face_analysis.py:775-800; FaceDetectUpdated.py:686), which crops every window with PIL's
 * Image.transform((w, h), EXTENT, (x0, y0, x1, y1), NEAREST).  Same index rule, bit for bit
 * (tested against PIL).  The *_rotate entries also take delta_angs (degrees, counter-clockwise, the
 * reference passes -1 * curr_angles, face_analysis.py:782; null = no rotation): a window with
 * delta_ang != 0 is cut from frame.rotate(delta_ang, NEAREST, center = centre of its box) — PIL's
 * Image.rotate arithmetic (16.16 fixed point), composed with the EXTENT rule per pixel; cuicuilco's own
 * composition is not available, this rule is the build's and is tested against PIL.
 * frame: (frame_h, frame_w) pixels, HG_U8 or HG_F32, row stride ld elements.  boxes: n x 4 doubles
 * (x0, y0, x1, y1) in frame coordinates.  out: n rows of out_w*out_h elements (row-major pixels,
 * the layout flow.execute expects), row stride ldo elements, dtype U8 / F32 / F64. */
typedef struct hg_patcher hg_patcher;
int hg_patcher_create(int device, hg_patcher** out);
void hg_patcher_free(hg_patcher* p);
int hg_patcher_extract_device(hg_patcher* p, const void* frame_dev, int frame_dtype, int frame_h, int frame_w,
                              int64_t ld, const double* boxes_dev, int64_t n, int out_w, int out_h,
                              void* out_dev, int out_dtype, int64_t ldo, void* stream);
/* The same for boxes the caller declares UNCHANGED between calls (key != 0; e.g. the prescale's whole-frame box, the first-stage
 * grid of a frame size, which depend on the frame's size only — face_analysis.py:630-669): the index tables are built on the first
 * call with a key (and whenever n or a size differs from what the key was built for) and reused afterwards.  Unrotated windows.
 * key = 0: hg_patcher_extract_device.
 * The contract the tables rest on:
 *  - THE KEY DETERMINES THE BOXES.  A table is found by (key, n, out_w, out_h, frame_w, frame_h); boxes_dev is read only when a
 *    table is built and never compared afterwards.  Two calls with equal key, n and sizes but different boxes get the first call's
 *    windows.  (The cascade hashes everything its boxes are computed from: the level table, or the frame and prescaled sizes.)
 *  - ONE STREAM PER PATCHER.  A patcher keeps four tables and replaces them round-robin, by a launch on the calling stream; only a
 *    table that has to grow waits for that stream first.  Calls on one patcher must therefore be ordered on one stream (or by the
 *    caller's own events): a launch on a second stream may read a table while it is rewritten.  More than four keys in rotation
 *    are correct but rebuild a table on every call. */
int hg_patcher_extract_keyed_device(hg_patcher* p, uint64_t key, const void* frame_dev, int frame_dtype, int frame_h, int frame_w,
                                    int64_t ld, const double* boxes_dev, int64_t n, int out_w, int out_h, void* out_dev,
                                    int out_dtype, int64_t ldo, void* stream);
int hg_patcher_extract(hg_patcher* p, const void* frame, int frame_dtype, int frame_h, int frame_w, int64_t ld,
                       const double* boxes, int64_t n, int out_w, int out_h, void* out, int out_dtype,
                       int64_t ldo);
int hg_patcher_extract_rotate_device(hg_patcher* p, const void* frame_dev, int frame_dtype, int frame_h, int frame_w,
                                     int64_t ld, const double* boxes_dev, const double* delta_angs_dev, int64_t n,
                                     int out_w, int out_h, void* out_dev, int out_dtype, int64_t ldo, void* stream);
int hg_patcher_extract_rotate(hg_patcher* p, const void* frame, int frame_dtype, int frame_h, int frame_w, int64_t ld,
                              const double* boxes, const double* delta_angs, int64_t n, int out_w, int out_h,
                              void* out, int out_dtype, int64_t ldo);
/* The same windows with PIL's interpolation filters (FaceDetectUpdated.py:125 chooses one per cascade stage).  The codes are PIL's
 * own, so a caller passes Image.BILINEAR straight through; any other code is HG_ERR_ARG.  filter = 0 is
 * hg_patcher_extract_rotate(_device), bit for bit.  BILINEAR / BICUBIC follow ImagingGenericTransform with affine_transform
 * (Geometry.c) for mode "L" images, every operation in double and rounded on its own:
 *   source point   xs = a0 (ox + 0.5) + a1 (oy + 0.5) + a2, ys likewise; outside [0, W) x [0, H) the pixel is 0; otherwise
 *                  x = floor(xs - 0.5), dx = (xs - 0.5) - x, the same for y.  EXTENT: a = ((x1-x0)/w, 0, x0, 0, (y1-y0)/h, y0).
 *   BILINEAR       2 x 2 taps, columns clipped, row y + 1 repeated from row y where it does not exist; (uint8) truncation.
 *   BICUBIC        a = -0.5, 4 x 4 taps, columns clipped, row y - 1 clipped, rows y .. y + 2 repeat the previous row's value where
 *                  they do not exist; <= 0 -> 0, >= 255 -> 255, else truncation.
 * A window with delta_ang % 360 != 0 is frame.rotate(delta_ang, F, center = box centre).transform((w, h), EXTENT, box, F) with the
 * SAME filter F in both steps (the build's choice, as for NEAREST: cuicuilco's composition is not available): the intermediate is a
 * uint8 image, each tap of the second step a filtered, quantised pixel of the rotated frame (0 where the rotation reads outside the
 * source).  The rotation uses the matrix Image.rotate builds as doubles (the 16.16 fixed point belongs to NEAREST: no range limit).
 * Frames: HG_U8 only — an HG_F32 frame with a filter other than NEAREST is HG_ERR_ARG (PIL's mode "F" rule is a different one).
 * Outputs: the uint8 value, converted to out_dtype.  Tested bit for bit against PIL. */
enum hg_filter { HG_FILTER_NEAREST = 0, HG_FILTER_BILINEAR = 2, HG_FILTER_BICUBIC = 3 };
int hg_patcher_extract_filter_device(hg_patcher* p, int filter, const void* frame_dev, int frame_dtype, int frame_h, int frame_w,
                                     int64_t ld, const double* boxes_dev, const double* delta_angs_dev, int64_t n, int out_w,
                                     int out_h, void* out_dev, int out_dtype, int64_t ldo, void* stream);
int hg_patcher_extract_filter(hg_patcher* p, int filter, const void* frame, int frame_dtype, int frame_h, int frame_w, int64_t ld,
                              const double* boxes, const double* delta_angs, int64_t n, int out_w, int out_h, void* out,
                              int out_dtype, int64_t ldo);

/* --- Colour frames: PIL's "L" conversion -----------------------------------------------------------------------------------
 * A camera or a decoder delivers packed colour pixels; the reference converts them first (im.convert("L"),
 * FaceDetectUpdated.py:541-543; its file branch loads with image_format="L", :533).  PIL's rule is integer and per pixel,
 *     L = (R * 19595 + G * 38470 + B * 7471 + 0x8000) >> 16
 * and a fourth byte (RGBA, RGBX) is ignored.  Tested bit for bit against PIL, every 24-bit colour included.
 * A colour frame is frame_h rows of frame_w packed pixels, rows ld_bytes BYTES apart: any ld_bytes >= frame_w * bytes per pixel
 * and any base address, so a crop of a larger colour frame is a frame.  HG_FRAME_L is the grey frame every other entry reads. */
#define HG_FRAME_L    0   /* one byte per pixel */
#define HG_FRAME_RGB  1   /* packed, 3 bytes per pixel */
#define HG_FRAME_BGR  2
#define HG_FRAME_RGBA 3   /* packed, 4 bytes per pixel, 4th byte ignored (RGBX too) */
#define HG_FRAME_BGRA 4
/* The whole frame -> dst_dev (frame_h rows of frame_w bytes, dst_ld >= frame_w apart), enqueued on `stream`, no host wait.
 * HG_FRAME_L: a pitched copy.  src and dst must NOT overlap (a thread reads four pixels and writes four bytes; nothing orders it
 * against its neighbours).  HG_ERR_ARG, nothing launched: unknown format, null pointer, frame_h / frame_w <= 0,
 * ld_bytes < frame_w * bytes per pixel, dst_ld < frame_w. */
int hg_frame_to_gray_device(int device, const void* src_dev, int format, int frame_h, int frame_w, int64_t ld_bytes,
                            uint8_t* dst_dev, int64_t dst_ld, void* stream);
/* The same rule on the host, no device involved (runs on a machine without a GPU). */
int hg_frame_to_gray_host(const void* src, int format, int frame_h, int frame_w, int64_t ld_bytes, uint8_t* dst, int64_t dst_ld);
/* NEAREST, unrotated windows cut straight from a colour uint8 frame: every output pixel is the conversion of the source pixel
 * hg_patcher_extract_device would pick on the converted frame (same index tables), 0 outside the frame.  Only the picked pixels
 * are read.  Rotated and BILINEAR / BICUBIC windows are not cut from colour: convert first.  HG_FRAME_L: hg_patcher_extract_device
 * on an HG_U8 frame. */
int hg_patcher_extract_format_device(hg_patcher* p, int frame_format, const void* frame_dev, int frame_h, int frame_w, int64_t ld_bytes,
                                     const double* boxes_dev, int64_t n, int out_w, int out_h, void* out_dev, int out_dtype,
                                     int64_t ldo, void* stream);

/* --- Antialiased resize: PIL's Image.resize((w, h), filter) ------------------------------------------------------------------
 * The prescale of every frame path is im.resize((w, h), Image.NEAREST) (FaceDetectUpdated.py:551-556): point sampling, which aliases; the
 * reference's author left the alternatives in a comment on that line and makes the display copy with BILINEAR (:559).  These entries
 * are Pillow's resize for 8-bit images (ImagingResample, Resample.c), bit for bit (tested against PIL).
 * enum hg_resample and enum hg_filter are DIFFERENT OPERATIONS that share PIL's codes: hg_filter is transform(EXTENT, filter), which
 * samples a fixed 2 x 2 / 4 x 4 neighbourhood of each source point (right for windows); hg_resample is a separable convolution whose
 * support grows with the shrink factor — that growth is the antialiasing.  On a 192 x 108 -> 100 x 56 noise image the two differ in
 * 5534 of 5600 pixels.  The rule, per axis that changes size (in -> out pixels; doubles, every operation rounded on its own):
 *   filters   BOX (support S = 0.5) 1 for -0.5 < x <= 0.5; BILINEAR (1) 1 - |x|; HAMMING (1) sinc(x) (0.54f + 0.46f cos(pi x)), the two
 *             constants being floats as Pillow writes them; BICUBIC (2) a = -0.5; LANCZOS (3) sinc(x) sinc(x / 3) for -3 <= x < 3
 *   tables    scale = in / out, fs = max(scale, 1), support = S fs, ksize = (int)ceil(support) * 2 + 1; for output pixel xx:
 *             center = (xx + 0.5) scale, xmin = max((int)(center - support + 0.5), 0), xmax = min((int)(center + support + 0.5), in) - xmin,
 *             w[x] = f((x + xmin - center + 0.5) / fs) for x < xmax, normalised by their running sum when that is not 0,
 *             k[x] = (int)(w[x] 2^22 -+ 0.5) (sin / cos: the host's libm, the one PIL calls on that machine)
 *   one pass  out[xx] = clip8((2^21 + sum_{x < xmax} in[xmin + x] k[x]) >> 22), int32, arithmetic shift, clamped to 0..255
 * The horizontal pass runs first (if the width changes) into a uint8 image, the vertical pass reads that (if the height changes); an
 * axis that keeps its size gets no pass.  Image.resize's own exception is kept: a very tall image (h > 100 w) whose height shrinks has
 * its height resized first, at full width, and its width afterwards.  out_format is HG_FRAME_L or the source's own format:
 *   grey output from a colour source   convert("L") of every source pixel read, then the passes (im.convert("L").resize(...), the
 *                                      reference's order, :543 then :556; the other order gives other bytes)
 *   colour output                      band by band with the same tables; the four-byte formats as RGBX, all four bytes (Pillow
 *                                      premultiplies mode "RGBA" proper before a filtered resize: not offered)
 * HG_RESAMPLE_NEAREST with grey output is the whole-frame gather the prescale has always used (hg_patcher_extract_format_device over
 * the box (0, 0, w, h)): the same bytes as before; with colour output it is refused.  Not offered: Pillow's box= and reducing_gap=.
 * HG_ERR_ARG with a message, before anything is launched or written: an unknown filter or format, an out_format that is neither
 * HG_FRAME_L nor the source's, null pointers, sizes <= 0, ld_bytes < w * bytes per pixel, dst_ld_bytes < out_w * bytes per output pixel,
 * NEAREST with colour output, source and destination whose byte ranges overlap, and an axis whose tables (out * (ksize + 2) int32)
 * exceed HG_RESAMPLE_MAX_TABLE_BYTES. */
enum hg_resample {
    HG_RESAMPLE_NEAREST = 0, HG_RESAMPLE_LANCZOS = 1, HG_RESAMPLE_BILINEAR = 2, HG_RESAMPLE_BICUBIC = 3, HG_RESAMPLE_BOX = 4, HG_RESAMPLE_HAMMING = 5
};
#define HG_RESAMPLE_MAX_TABLE_BYTES (64 << 20)
/* The rule on the host, plain C++, no device involved: src is h rows of w pixels of `format`, ld_bytes apart; dst out_h rows of out_w
 * pixels of out_format, dst_ld_bytes apart. */
int hg_frame_resize_host(int filter, const void* src, int format, int h, int w, int64_t ld_bytes, int out_format, void* dst, int out_h,
                         int out_w, int64_t dst_ld_bytes);
/* The same on the patcher's device, enqueued on `stream`, no host wait.  Rows may start at any byte; no load touches a byte outside
 * [row start, row start + w * bytes per pixel).  The patcher keeps the uploaded tables of the eight most recently used (in, out, filter) axes and the
 * intermediate image; both grow on demand, so from the second frame of a size a call uploads and allocates nothing.  ONE STREAM PER
 * PATCHER, as for the keyed tables above.  A MISS IS A HOST WAIT: the tables of an axis the patcher does not hold are computed on the
 * host, and when they replace another axis' (the least recently used of eight) the call first waits for the calling stream; so is an
 * intermediate that has to grow.  A caller that alternates more than four (size, filter) pairs through one patcher pays that on every
 * call — inside hg_cascade_detect_frame_device and the tracker steps too, when a filter is set and frame sizes rotate.
 * Two launches (horizontal, then vertical; the horizontal pass writes only the source rows the vertical pass reads), or ONE where both
 * axes change and a 64 x 16 output tile's intermediate rows fit the kernel's 16 KB of LDS: the same bytes.  Which sources and filters take the
 * one launch by default follows the measurement (hg_resample.hip, kFusedDefault).  flags: bit 0 forces the two launches, bit 1 the one
 * launch where it is eligible (both for tests and A/B runs; not both at once); other bits must be 0.  Rows of at most 2^28 pixels;
 * NEAREST writes at most 4096 x 4096 pixels (the window gather's limit). */
int hg_patcher_resize_device(hg_patcher* p, int filter, int flags, const void* src_dev, int format, int h, int w, int64_t ld_bytes,
                             int out_format, void* dst_dev, int out_h, int out_w, int64_t dst_ld_bytes, void* stream);

/* --- Pose-normalised face crops: face_normalization_tools.normalize_image ---------------------------------------------------------
 * What the reference does with the purged rows next (face_analysis.py:983-1013, 256 x 192 crops from approximate eyes; :1170-1222,
 * 256 x 260 crops from the located eyes, the input of age / race / gender estimation): normalize_image (face_normalization_tools.py:111-329)
 * for the one configuration both callers use — centering_mode "mid_eyes_inferred-mouth", rotation_mode "EyeLineRotation" or "noRotation",
 * integer_rotation_center, no random background, mode "L", the mouth inferred from the eyes, and the scale methods
 * "eyes_inferred-mouth_area" / "eyes_inferred-mouth_areaZ".  Bit for bit against PIL.
 * Geometry, per face on the HOST, float64, the reference's operation order, one rounding per operation, the host's libm (the one Python's
 * math uses), from eyes (lx, ly, rx, ry) in the coordinates of the frame passed in and its size (fw, fh):
 *   exm = (rx + lx) / 2, eym = (ry + ly) / 2; dist = sqrt((lx - rx)^2 + (ly - ry)^2); eye_line_angle = atan2(ry - ly, rx - lx) * 180 / pi
 *   mouth  mx = exm - (42 / 37)(ry - ly), my = eym + (42 / 37)(rx - lx); height = sqrt((exm - mx)^2 + (eym - my)^2); area = dist height / 2
 *   scale  = sqrt(area / (37 * 42 / 2 * (37.5 / 37)^2)); ori_w = out_w scale, ori_h = out_h scale, each / 2 for areaZ
 *   centre cx = (exm + mx) / 2, cy = (eym + my) / 2; cxi = (int)(cx + 0.5), cyi = (int)(cy + 0.5) (truncation)
 *   crop   W = (int)(2 max(fw - 1 - cxi + 0.5, cxi + 0.5) + 0.5), H likewise (both odd); crop_x0 = cxi - (W - 1) / 2, crop_y0 likewise
 *   angle  = eye_line_angle, or 0 when consts.rotate == 0; rad = -angle * pi / 180; Dx = cx - cxi, Dy = cy - cyi;
 *          shift = (Dx cos(rad) - Dy sin(rad), Dy cos(rad) + Dx sin(rad))
 *   box    ncx = (W - 1) / 2 + shift[0], ncy likewise; (ncx - (ori_w - 1) / 2, ncy - (ori_h - 1) / 2, ncx + (ori_w - 1) / 2 + 1, ncy + (ori_h - 1) / 2 + 1)
 *   m      the matrix Image.rotate(angle) builds on a W x H image, default centre (W / 2, H / 2): round(cos, 15), round(sin, 15) of
 *          -radians(angle % 360.0), m2 = m0 (-W / 2) + m1 (-H / 2) + 0 + W / 2, m5 likewise; rotated = 0 where angle % 360.0 == 0 (m the identity)
 * Pixels, PIL composed as the reference composes it:
 *   crop = im.transform((W, H), EXTENT, (crop_x0, crop_y0, crop_x0 + W, crop_y0 + H))      NEAREST, an integer box: a shift, 0 outside the frame
 *   rot  = crop.rotate(angle, BICUBIC)                                                     the rule this build owns for cuicuilco's rotate_improved
 *   out  = rot.transform((out_w, out_h), EXTENT, box, BICUBIC)
 * with the BICUBIC arithmetic of hg_patcher_extract_filter_device above, applied RELATIVE TO THE CROP: clipping and the outside test use
 * W x H, the crop's zero padding takes part in the taps, rot is uint8.  Only the rectangle of rot the final cut reads is ever computed
 * (rect: columns x - 1 .. x + 2 of every output column that is inside, clipped to [0, W); rows likewise); the crop is never materialised.
 * status, per face (a refused face has an all-zero image and geom; its neighbours are untouched; never an error of the whole call):
 *   HG_NORM_OK 0; HG_NORM_EYES_SWAPPED 1: lx > rx (the reference exits); HG_NORM_NOT_FINITE 2: a coordinate, or the eye distance computed from them, is not finite;
 *   HG_NORM_ZERO_DISTANCE 3: dist == 0; HG_NORM_CENTRE_RANGE 4: |cx| or |cy| above 2^20 (guards the int conversion). */
#define HG_NORM_AREA  0   /* "eyes_inferred-mouth_area"  */
#define HG_NORM_AREAZ 1   /* "eyes_inferred-mouth_areaZ": ori_w / 2, ori_h / 2 */
enum hg_norm_status { HG_NORM_OK = 0, HG_NORM_EYES_SWAPPED = 1, HG_NORM_NOT_FINITE = 2, HG_NORM_ZERO_DISTANCE = 3, HG_NORM_CENTRE_RANGE = 4 };
typedef struct hg_norm_consts {
    int32_t out_w, out_h;     /* 1 .. 4096 each */
    int32_t method;           /* HG_NORM_AREA / HG_NORM_AREAZ */
    int32_t rotate;           /* 1: EyeLineRotation, 0: noRotation */
} hg_norm_consts;
typedef struct hg_norm_geom {
    int32_t crop_x0, crop_y0, W, H;
    double angle;
    double shift[2];          /* Delta_x_rotated, Delta_y_rotated */
    double m[6];
    double box[4];
    int32_t rotated, status;
    int32_t rect[4];          /* x0, y0, width, height of the part of rot the cut reads (width = height = 0: no output pixel is inside) */
} hg_norm_geom;
/* eyes: (n, 4) doubles; geoms_out: n records.  HG_ERR_ARG: null pointers with n > 0, n < 0, out_w / out_h outside 1 .. 4096, an unknown
 * method, rotate not 0 / 1, frame_w / frame_h outside 1 .. 2^24.  Plain C++, no device. */
int hg_normalize_geometry_host(const double* eyes, int64_t n, int frame_w, int frame_h, const hg_norm_consts* consts, hg_norm_geom* geoms_out);
/* The whole pixel rule on the host (no device): frame is frame_h rows of frame_w grey bytes, ld >= frame_w apart, any base address;
 * out is n images of out_h x out_w bytes, ldo >= out_w * out_h apart.  Refusals as for the device entry below. */
int hg_normalize_faces_host(const uint8_t* frame, int frame_h, int frame_w, int64_t ld, const hg_norm_geom* geoms, int64_t n, int out_w, int out_h,
                            uint8_t* out, int64_t ldo);
/* The same on the patcher's device, enqueued on `stream`, no host wait; geoms_host is consumed before the call returns.  Grey uint8
 * frames only (a colour frame goes through hg_frame_to_gray_device first).  All launch and scratch sizes come from the geoms.
 *   staged       pass A computes every pixel of a face's rect ONCE into per-face scratch (uint8), pass B is the BICUBIC cut from it
 *   tap by tap   a face whose rect holds more pixels than the cut has taps (16 out_w out_h: shrunk more than about 4 x per axis) computes
 *                each tap's rotated pixel where it is used; no scratch.  Scratch is so at most 16 out_w out_h bytes per face.
 * Both give the same bytes.  flags: bit 0 forces staging (refused, HG_ERR_ARG, if a rect exceeds 2^26 pixels), bit 1 forces tap by tap
 * (for tests and A/B runs; not both); other bits must be 0.  The face records and the scratch live with the patcher and grow on demand
 * (growing waits for `stream`); ONE STREAM PER PATCHER, as for the other entries.
 * HG_ERR_ARG, nothing launched: a null pointer, a non-positive size, out_w / out_h above 4096, ld < frame_w, ldo < out_w * out_h, n < 0,
 * a geom whose W / H disagree with the frame size (W != 2 max(frame_w - 1 - cxi, cxi) + 1 for cxi = crop_x0 + (W - 1) / 2) or whose rect
 * leaves [0, W) x [0, H).  n == 0: HG_OK, nothing launched.  Faces with status != 0 get an all-zero image. */
int hg_patcher_normalize_device(hg_patcher* p, int flags, const uint8_t* frame_dev, int frame_h, int frame_w, int64_t ld,
                                const hg_norm_geom* geoms_host, int64_t n, int out_w, int out_h, uint8_t* out_dev, int64_t ldo, void* stream);

/* --- Cascade glue on the device (the reference's stage loop between two hot calls) -----------------
 * update_current_subimage_coordinates (face_analysis.py:803-840) + identify_patches_to_discard (:842-887) for n
 * candidates from their regression outputs, then the boolean-mask compaction of FaceDetectUpdated.py:739-759 as
 * "index map + row gather", so that extract -> execute -> regression -> update -> discard -> compaction chain on one
 * stream.  float64, the reference's operation order.  Candidates of all pyramid levels may share a batch: the per-level
 * constants travel per ORIGINAL window in orig_level (n0, 3) = (max_Dx_diff, max_Dy_diff, base_side),
 * FaceDetectUpdated.py:595,604-605; orig_index maps a candidate to its original window (:621). */
enum hg_stage_type { HG_STAGE_DISC = 0, HG_STAGE_POSX = 1, HG_STAGE_POSY = 2, HG_STAGE_PANG = 3, HG_STAGE_SCALE = 4 };
typedef struct hg_cascade_consts {
    double regression_width, regression_height;   /* Pipeline header (face_analysis.py:395-400)            */
    double desired_sampling;                      /* 0.825 (FaceDetectUpdated.py:729)                        */
    double tolerance_posxy_deviation, tolerance_scale_deviation, tolerance_angle_deviation; /* :113-115      */
    double max_scale_radio, min_scale_radio;      /* net_maxs / 0.825, net_mins / 0.825 (:596-597)           */
    double net_Dang;
    double cut_off_face;                          /* cut_offs_face[network_serial] (:98, :672), Disc stages  */
} hg_cascade_consts;
/* coords (n,4) and angles (n) are updated in place; discard[i] = 1 where the reference sets new_wrong_images. */
int hg_cascade_update_device(int device, int stage_type, const hg_cascade_consts* c, int64_t n, double* coords_dev,
                             double* angles_dev, const double* reg_dev, const int32_t* orig_index_dev,
                             const double* orig_coords_dev, const double* orig_angles_dev, const double* orig_level_dev,
                             uint8_t* discard_dev, void* stream);
/* map_dev[j] = index of the j-th candidate with discard == 0 (order kept), *count_dev = how many. */
int hg_cascade_compact_device(int device, const uint8_t* discard_dev, int64_t n, int32_t* map_dev, int32_t* count_dev,
                              void* stream);
/* dst[j, :] = src[map[j], :] for j < *count_dev (count read on the device); rows of row_bytes bytes (multiple of 4);
 * n_max bounds the launch (the candidate count before compaction).  Out of place. */
int hg_gather_rows_device(int device, const void* src_dev, void* dst_dev, int64_t row_bytes, const int32_t* map_dev,
                          const int32_t* count_dev, int64_t n_max, void* stream);

/* The whole stage loop (FaceDetectUpdated.py:665-766) of one batch of first-stage windows as ONE host call: for every stage
 * extract (rotated by -angle, unless the previous stage was a Disc stage or the stage has no network, :674-681) -> the stage's
 * flow (hg_flow_execute_device; NULL = reuse the previous features, the pipeline's "None0") -> regression -> coordinate update,
 * discard test, compaction (one fused kernel).  A stage that owns a network and the stages behind it whose network is NULL (at most
 * four) read the same sl: they run as ONE regression launch (hg_gauss_regression_multi_device) and ONE glue launch that applies
 * their updates and discard tests per row in stage order — same survivors, same order, same bits (HIGSFA_CASCADE_NO_GROUPS=1:
 * one stage per launch).  No per-candidate array visits the host; the host reads the survivor count only
 * after Disc stages (where it shrinks a lot and sizes the next launches) — between them launches are sized by the last count
 * read and the kernels take the exact count from device memory.  All pyramid levels may be one batch (:599).
 * flow / classifier handles stay owned by the caller and must live on `device`. */
typedef struct hg_gauss hg_gauss;
typedef struct hg_cascade hg_cascade;
typedef struct hg_cascade_stage {
    int32_t type;            /* enum hg_stage_type                                                   */
    int32_t serial;          /* trailing digit of the stage name: index into cut_offs_face (:669-672) */
    hg_flow* flow;           /* NULL: networks[k] is None                                            */
    hg_gauss* classifier;
} hg_cascade_stage;
int hg_cascade_create(const hg_cascade_stage* stages, int n_stages, int sub_w, int sub_h, int n_features,
                      const hg_cascade_consts* consts, const double* cut_offs_face, int n_cut_offs, int device,
                      hg_cascade** out);
void hg_cascade_free(hg_cascade* c);
/* The interpolation filter of every stage's extraction (enum hg_filter), indexed by the stage's serial exactly like cut_offs_face:
 * interpolation_formats[network_serial], FaceDetectUpdated.py:125, :671, :686.  HG_ERR_ARG (and nothing changed) if a stage's
 * serial is >= n or a code is unknown.  Before the first call every stage is NEAREST.  A stage that skips its extraction (the stage
 * before it is a Disc stage, or it has no network, :674-684) reuses the previous patches: its entry has no effect, as in the
 * reference.  The prescale is not a stage: it keeps its own filter (hg_cascade_set_prescale_filter; NEAREST until set, :551-561).  Takes effect from the next detect / step call on this handle; setting it
 * while a call on this handle is in flight on another thread or stream is the caller's error. */
int hg_cascade_set_interpolation(hg_cascade* c, const int32_t* filters, int n);
/* The format of the frames handed to this cascade (HG_FRAME_*; HG_FRAME_L until set).  Afterwards frame_dev / ld of
 * hg_cascade_detect_device, hg_cascade_detect_levels_device, hg_cascade_detect_frame_device, hg_cascade_detect_faces_frame_device
 * and hg_tracker_step_frame_device (a tracker on this cascade) are read as that format, ld in BYTES (for HG_FRAME_L what it always
 * meant), and refused with HG_ERR_ARG for ld < frame_w * bytes per pixel.  With a prescale the grey prescaled frame is cut from the
 * colour frame in one launch that reads the sampled pixels only; without one the frame is converted once into a grey buffer that
 * lives with the cascade and grows on demand.  Everything behind that — the grid, the stage loop, the eye step, the purge, the
 * tracker — reads that grey frame.  May be called between frames, like hg_cascade_set_interpolation; HG_ERR_ARG (and nothing
 * changed) for an unknown format. */
int hg_cascade_set_frame_format(hg_cascade* c, int format);
/* The filter of the prescale (enum hg_resample — NOT enum hg_filter; HG_RESAMPLE_NEAREST until set): with any other filter the prescale of
 * hg_cascade_detect_frame_device, hg_cascade_detect_faces_frame_device and both tracker steps is hg_patcher_resize_device on the cascade's
 * patcher — im.convert("L").resize((w, h), filter) — into the same cascade-owned grey buffer; the grid, the stage loop, the eye step and the
 * tracker read that frame as before.  A handle never given a filter, or set back to NEAREST, runs exactly the launches it always ran.
 * May be called between frames, like hg_cascade_set_interpolation; HG_ERR_ARG (and nothing changed) for an unknown code. */
int hg_cascade_set_prescale_filter(hg_cascade* c, int filter);
/* frame_dev: (frame_h, frame_w) uint8 on the device, row stride ld >= frame_w (a pitched buffer, a crop of a larger frame); this
 * and every entry below that reads a frame returns HG_ERR_ARG for ld < frame_w before it launches or writes anything; boxes_host (n0, 4) / level_host (n0, 3): the first-stage
 * windows and their level constants.  Outputs (host, room for out_cap detections): final coordinates, angles, index of the
 * original window, Disc confidence; *n_out detections; stage_counts[n_stages] survivors after each stage (-1 where the count
 * was not read back); *rows_executed rows pushed through flows.  Synchronous. */
int hg_cascade_detect_device(hg_cascade* c, const void* frame_dev, int frame_h, int frame_w, int64_t ld,
                             const double* boxes_host, const double* level_host, int64_t n0, double* out_coords,
                             double* out_angles, int32_t* out_orig_index, double* out_confidence, int64_t out_cap,
                             int64_t* n_out, int32_t* stage_counts, int64_t* rows_executed, void* stream);

/* The same with the first-stage windows computed ON THE DEVICE from the grid's closed form (face_analysis.py:630-646, :661-669):
 * pyramid level L holds ny x nx windows, y-major, at numpy.linspace(0, stop, n) positions; a window is
 * (posX, posY, posX + patch_w - 1, posY + patch_h - 1); every window of the level carries (max_dx, max_dy, base_side)
 * (face_analysis.py:651-652, FaceDetectUpdated.py:604-605).  float64 in numpy's operation order: the boxes equal the host
 * formulas' bit for bit (hg_cascade_grid_device writes them to device arrays for inspection; boxes_dev == NULL: only *n0). */
typedef struct hg_cascade_level {
    int32_t nx, ny;                      /* grid points along x / y (face_analysis.py:640-641)            */
    double x_stop, y_stop;               /* im_width - patch_w, im_height - patch_h (end points, :645-646) */
    double patch_w, patch_h;             /* subimage size x sampling value (:630-631)                      */
    double max_dx, max_dy, base_side;    /* net_Dx * patch_w / regression_width, ..., sqrt(pw^2 + ph^2)    */
} hg_cascade_level;
int hg_cascade_detect_levels_device(hg_cascade* c, const void* frame_dev, int frame_h, int frame_w, int64_t ld,
                                    const hg_cascade_level* levels, int n_levels, double* out_coords, double* out_angles,
                                    int32_t* out_orig_index, double* out_confidence, int64_t out_cap, int64_t* n_out,
                                    int32_t* stage_counts, int64_t* rows_executed, void* stream);
/* One frame, one host call: the reference's prescale (im.resize((w, h), NEAREST), FaceDetectUpdated.py:551-561; prescale_w = 0: none)
 * into a buffer owned by the cascade, the grid of the PRESCALED frame from `levels`, the stage loop. */
int hg_cascade_detect_frame_device(hg_cascade* c, const void* frame_dev, int frame_h, int frame_w, int64_t ld, int prescale_w,
                                   int prescale_h, const hg_cascade_level* levels, int n_levels, double* out_coords,
                                   double* out_angles, int32_t* out_orig_index, double* out_confidence, int64_t out_cap,
                                   int64_t* n_out, int32_t* stage_counts, int64_t* rows_executed, void* stream);
int hg_cascade_grid_device(int device, const hg_cascade_level* levels, int n_levels, double* boxes_dev, double* level_dev,
                           int64_t cap, int64_t* n0, void* stream);

/* --- Eye localisation and duplicate purge after the face cascade (FaceDetectUpdated.py:947-1041, :1180) -------------------
 * For the survivors of one frame (boxes (n,4), angles (n)), on the frame the cascade read:
 *   eye boxes      compute_approximate_eye_boxes_coordinates(box, 0.825, 2.3719, rot_angle=angle) (face_analysis.py:61-133), float64
 *                  in its own operation order; left boxes are rows 0..n-1 of every 2n-row intermediate, right boxes rows n..2n-1.
 *                  The right eye goes through the left eye's procedure unchanged (find_Right_eyes, face_analysis.py:1022-1033,
 *                  passes the unswapped box with left_eye=1; the swap back cannot move the box centre).
 *   patches        eye_w x eye_h windows rotated by delta_ang = -angle, the patcher's NEAREST / EXTENT rule, then the contrast
 *                  step: per patch, from exact int64 sums S1 = sum p, S2 = sum p^2 over N = w*h pixels (zeros outside the frame),
 *                  mean = S1/N, std = sqrt((N*S2 - S1^2) / (N*N)); p' = clip((p - mean) / (std / target_std + 1e-8) + target_mean,
 *                  0, 255) as float32 (image_array_contrast_normalize_avg_std, face_analysis.py:318-327; the mapping of the
 *                  reference's obj_avg / obj_std to pixel units is not known: the targets are the caller's).
 *   networks       EyeLX / EyeLY (networks[num_networks-5], [num_networks-4]): one hg_flow_execute_device over the 2n rows when
 *                  both stages name one flow, then one hg_gauss_regression_multi_device for both classifiers.
 *   too far        |reg| >= tolerance for either classifier and either eye (face_analysis.py:1073).
 *   shift          reg / eye_sampling * box side / regression size, rotated by -angle, subtracted from the eye box; the eye is the
 *                  box centre (face_analysis.py:1075-1104, FaceDetectUpdated.py:1008-1009). */
typedef struct hg_eyes hg_eyes;
typedef struct hg_eye_consts {
    double eye_regression_width, eye_regression_height;  /* Pipeline header line 3: 64 64 (face_analysis.py:395-400)      */
    double face_sampling, eye_sampling;                   /* 0.825, 2.3719 (FaceDetectUpdated.py:948, :1074-1082)          */
    double tolerance;                                     /* tolerance_xy_eye 9.0 (face_analysis.py:1018)                  */
    double target_mean, target_std;                       /* contrast targets in pixel units: required, no default          */
    int32_t eye_w, eye_h;                                 /* eye_subimage_width x eye_subimage_height: 64 x 64              */
    int32_t n_features;                                   /* feature columns kept per row (>= both classifiers' input_dim) */
    int32_t reserved;                                     /* 0                                                              */
} hg_eye_consts;
/* flow_x / flow_y must live on `device` (they run with float32 output), input width eye_w * eye_h; the classifiers on `device`
 * with input_dim <= n_features.  HG_ERR_ARG / HG_ERR_DIM on a violation.  The handles stay owned by the caller. */
int hg_eyes_create(hg_flow* flow_x, hg_gauss* clf_x, hg_flow* flow_y, hg_gauss* clf_y, const hg_eye_consts* consts, int device,
                   hg_eyes** out);
void hg_eyes_free(hg_eyes* e);
/* The filter of the eye patches (enum hg_filter; NEAREST until set): the reference hands find_Left_eyes / find_Right_eyes whatever
 * the stage loop's last iteration left in interpolation_format (FaceDetectUpdated.py:671, :994, :1001).  The contrast step after the
 * gather is unchanged.  HG_ERR_ARG for an unknown code.  Takes effect from the next call on this handle; setting it while a call on
 * this handle is in flight on another thread or stream is the caller's error. */
int hg_eyes_set_interpolation(hg_eyes* e, int filter);
/* The eye step for n faces, BEFORE the discard: frame_dev (h, w) uint8 on the device, row stride ld; boxes_dev (n,4) and angles_dev (n)
 * float64 on the device.  Outputs (device): eye_coords_dev (n,4) = (eyeL_x, eyeL_y, eyeR_x, eyeR_y), too_far_dev (n) 0/1;
 * patches_dev (nullable) the contrast-normalised patches (2n, eye_w*eye_h) float32; reg_dev (nullable) the regressions (2, 2n) float64,
 * row 0 EyeLX, row 1 EyeLY.  Enqueued on `stream`. */
int hg_eyes_locate_device(hg_eyes* e, const void* frame_dev, int frame_h, int frame_w, int64_t ld, const double* boxes_dev,
                          const double* angles_dev, int64_t n, double* eye_coords_dev, uint8_t* too_far_dev, float* patches_dev,
                          double* reg_dev, void* stream);
/* The eye boxes alone (the first step of hg_eyes_locate_device, exported for callers that drive the steps themselves): eye_boxes_dev
 * (2n, 4) float64, left boxes then right boxes; delta_angs_dev (nullable, 2n) the rotation their patches are cut with (-angle). */
int hg_eyes_boxes_device(hg_eyes* e, const double* boxes_dev, const double* angles_dev, int64_t n, double* eye_boxes_dev, double* delta_angs_dev,
                         void* stream);
/* purgue_detected_faces_angles_eyes_confidence (face_analysis.py:186-221) on the device, one workgroup: rows_dev (n,10) float64
 * (x0, y0, x1, y1, angle, eyeL_x, eyeL_y, eyeR_x, eyeR_y, confidence).  w = (1 - conf) * |eyeR - eyeL|, w / max(w); rows in the order
 * of numpy.argsort(w, kind="stable")[::-1] (NaN first; the reference's argsort is not stable, the build pins this tie rule); the
 * greedy pass keeps a row whose smallest relative_error_detection against the rows kept so far is > 0.25, IEEE semantics.
 * out_rows_dev receives the kept rows in order and needs room for n + 1 rows (the reference's loop appends its first row a second
 * time when that row's eye distance is zero); *count_dev (device int32) their number.  Synchronous (it owns a scratch buffer). */
int hg_purge_detections_device(int device, const double* rows_dev, int64_t n, double* out_rows_dev, int32_t* count_dev, void* stream);
/* One frame, one host call: hg_cascade_detect_frame_device's prescale, grid and stage loop, then the eye step on the survivors (on the
 * frame the cascade read), the discard of the too-far faces (order kept), the row assembly and the purge.  The host reads nothing
 * between the cascade's last survivor count and the final count.  out_rows (host): room for out_cap faces of 10 doubles; the call fails
 * with HG_ERR_ARG, writing no row, when more faces remain.  *n_before_purge: faces after the discard.  Synchronous. */
int hg_cascade_detect_faces_frame_device(hg_cascade* c, hg_eyes* e, const void* frame_dev, int frame_h, int frame_w, int64_t ld,
                                         int prescale_w, int prescale_h, const hg_cascade_level* levels, int n_levels, double* out_rows,
                                         int64_t out_cap, int64_t* n_out, int64_t* n_before_purge, int32_t* stage_counts,
                                         int64_t* rows_executed, void* stream);

/* --- A stack of same-size frames through one pooled pass (the reference's batch mode: many images, one set of networks) -----
 * One frame's windows do not fill the device; the windows of B frames of ONE size are one batch.  Every row of the cascade is
 * independent of its batch and every compaction keeps row order, so each result below is DEFINED as what the per-frame entry returns
 * for that frame, bit for bit (tests/test_frame_batch_gpu.py).
 *
 * The patcher: row i is the window boxes_dev[i], rotated by delta_angs_dev[i] if given, cut from frame row_frame_dev[i] of a stack of
 * n_frames grey uint8 frames, all frame_h x frame_w with row stride ld, frame f starting frame_stride BYTES behind frame f - 1 — any
 * value >= (frame_h - 1) ld + frame_w, not necessarily a multiple of ld: the frames may be slices of a larger buffer.  Rule, tables and
 * bytes are those of hg_patcher_extract_filter_device on that one frame (NEAREST, BILINEAR, BICUBIC; rotated or not; any out_dtype).
 * A row whose frame index lies outside [0, n_frames) is an all-zero window; no address is formed from such an index.
 * HG_ERR_ARG, nothing launched and neither the handle nor a data pointer dereferenced: a null pointer (delta_angs_dev and stream may be
 * null), n_frames < 1, frame_stride below the bound, ld < frame_w, n < 0, an unknown filter, a bad output size / dtype / ldo.  n == 0:
 * HG_OK.  Enqueued on `stream`. */
int hg_patcher_extract_frames_device(hg_patcher* p, int filter, const void* frames_dev, int n_frames, int64_t frame_stride, int frame_h,
                                     int frame_w, int64_t ld, const double* boxes_dev, const double* delta_angs_dev,
                                     const int32_t* row_frame_dev, int64_t n, int out_w, int out_h, void* out_dev, int out_dtype, int64_t ldo,
                                     void* stream);
/* hg_cascade_detect_frame_device for a stack: frames_dev is frame 0 of n_frames frames in the cascade's frame format, frame_stride
 * and ld in bytes for a colour format as for the other entries.  Each frame is prescaled / converted by the code a single frame runs
 * (one pass per frame, the configured prescale filter) into a cascade-owned grey stack; grey frames without a prescale are read in
 * place.  The grid of the prescaled size is laid out once (n0 windows) and the candidates are n_frames copies of it: window f n0 + j is
 * window j of frame f.  The stage loop is the one loop — groups, the count read after Disc groups, the chunked glue above 8192
 * candidates — on n_frames n0 candidates.  Survivors come out ordered by frame and, within a frame, in that frame's own order:
 * frame f's are rows frame_first[f] .. frame_first[f + 1] (frame_first: n_frames + 1 entries, host), out_orig_index the index within
 * the frame's grid.  stage_counts / *rows_executed: the pooled totals — the sum of the per-frame counts where those are read, -1 where
 * they are not (a single frame that has run out of candidates reports 0 for the stages behind without reading anything; pooled, such a
 * stage is -1 as long as another frame has candidates).  HG_ERR_ARG before anything is launched or written: n_frames < 1 or > HG_MAX_STACK_FRAMES, n_frames n0 above the window
 * bound of the other entries (2^31 / 64), a bad frame geometry (as the other entries, and frame_stride below
 * (frame_h - 1) ld + frame_w bytes-per-pixel), a null frame_first.  Frames of different sizes do not share a call.  Synchronous. */
#define HG_MAX_STACK_FRAMES 1024
int hg_cascade_detect_frames_device(hg_cascade* c, const void* frames_dev, int n_frames, int64_t frame_stride, int frame_h, int frame_w,
                                    int64_t ld, int prescale_w, int prescale_h, const hg_cascade_level* levels, int n_levels,
                                    double* out_coords, double* out_angles, int32_t* out_orig_index, double* out_confidence, int64_t out_cap,
                                    int32_t* frame_first, int32_t* stage_counts, int64_t* rows_executed, void* stream);
/* hg_cascade_detect_faces_frame_device for a stack: the pooled stage loop, then the eye step on ALL survivors as one batch (every eye
 * row cut from its face's frame), the discard and the row assembly, and the purge PER FRAME — it is a per-image rule — one workgroup per
 * frame over that frame's rows.  out_rows: the kept rows ordered by frame, frame f's at frame_first[f] .. frame_first[f + 1];
 * n_before_purge (n_frames entries): faces of every frame after the discard.  The host reads nothing between the stage loop's last
 * survivor count and the one read-back of counts and rows.  HG_ERR_ARG, writing no row, when out_cap is below the kept total (a frame
 * may keep its count + 1).  Refusals as above.  Synchronous. */
int hg_cascade_detect_faces_frames_device(hg_cascade* c, hg_eyes* e, const void* frames_dev, int n_frames, int64_t frame_stride, int frame_h,
                                          int frame_w, int64_t ld, int prescale_w, int prescale_h, const hg_cascade_level* levels,
                                          int n_levels, double* out_rows, int64_t out_cap, int32_t* frame_first, int32_t* n_before_purge,
                                          int32_t* stage_counts, int64_t* rows_executed, void* stream);

/* --- A LIST of frames of different sizes through one pooled pass (a folder of photographs, cameras of different resolutions) --------
 * The stack entries above take frames of one size.  These take a list: every frame brings its own pointer, size and row stride, and —
 * in the cascade — its own prescaled size and level table.  The candidates are the CONCATENATION of the frames' grids: with n0_f the
 * windows of frame f's level table and first[f] = n0_0 + ... + n0_{f-1}, window first[f] + j is window j of frame f.  As for the stack,
 * each result is DEFINED as what the per-frame entry returns for that frame, bit for bit (tests/test_frame_list_gpu.py).  Frames of
 * ONE size stay the stack entries' case: those copy one grid and need no per-box descriptor.
 *
 * The descriptor arrays (hg_frame_ref, hg_cascade_frame, and the level tables they point to) are HOST memory, consumed before the call
 * returns: the caller may reuse them at once.
 *
 * The patcher: hg_patcher_extract_frames_device with the frame of row i described by frames[row_frame_dev[i]] — grey uint8, frame_h x
 * frame_w, rows ld bytes apart, anywhere in device memory.  Rule, tables and bytes are those of hg_patcher_extract_filter_device on that
 * one frame; a row whose frame index lies outside [0, n_frames) is an all-zero window and forms no address from the index.
 * HG_ERR_ARG, nothing launched and neither the handle nor a data pointer dereferenced: a null pointer (delta_angs_dev and stream may be
 * null), n_frames < 1 or > HG_MAX_STACK_FRAMES, ANY frame with frame_h <= 0, frame_w <= 0, ld < frame_w or a null frame_dev — the
 * message names the frame, and one bad frame refuses the whole call —, a rotated NEAREST call with a frame of 32768 pixels or more per
 * side, n < 0, an unknown filter, a bad output size / dtype / ldo.  n == 0: HG_OK.  Enqueued on `stream`. */
typedef struct hg_frame_ref {
    const void* frame_dev;
    int32_t frame_h, frame_w;
    int64_t ld;
} hg_frame_ref;
typedef struct hg_cascade_frame {
    const void* frame_dev;          /* in the cascade's frame format; ld in bytes */
    int32_t frame_h, frame_w;
    int64_t ld;
    int32_t prescale_w, prescale_h; /* 0, 0: none */
    const hg_cascade_level* levels; /* the grid of the (prescaled) frame */
    int32_t n_levels;
} hg_cascade_frame;
int hg_patcher_extract_frame_list_device(hg_patcher* p, int filter, const hg_frame_ref* frames, int n_frames, const double* boxes_dev,
                                         const double* delta_angs_dev, const int32_t* row_frame_dev, int64_t n, int out_w, int out_h,
                                         void* out_dev, int out_dtype, int64_t ldo, void* stream);
/* hg_cascade_detect_frames_device for a list.  Each frame is prescaled / converted by the code a single frame runs, to ITS prescaled
 * size, into its own slot of one cascade-owned grey buffer; a grey frame without a prescale is read where it is.  One kernel lays out
 * the concatenated grids from a device array of the DISTINCT level tables, with hg_cascade_grid_device's arithmetic.  The stage loop is
 * the one loop on the sum of the n0_f candidates; every extraction takes the row's frame from a per-window frame array.  First-stage
 * index tables: frames whose prescaled size and level table are equal share one set, all sets in one buffer that lives for the call.
 * Outputs as for the stack: survivors ordered by frame, frame_first (n_frames + 1), out_orig_index within the frame's own grid,
 * stage_counts / *rows_executed by the pooled rule.  HG_ERR_ARG before anything is launched or written: a null c / frames /
 * frame_first, n_frames < 1 or > HG_MAX_STACK_FRAMES, out_cap < 0, and for ANY frame (the message names it) a bad geometry (frame_h <=
 * 0, frame_w <= 0, ld < frame_w bytes-per-pixel), a null frame_dev, null levels, n_levels outside 1..32, a bad prescale size, 32768
 * pixels or more per side under its grid where a later NEAREST stage (or the NEAREST eye step of the faces entry) cuts rotated windows
 * from it; a total window count above 2^31 / 64.  HG_ERR_ARG when out_cap is below the survivors.  Synchronous. */
int hg_cascade_detect_frame_list_device(hg_cascade* c, const hg_cascade_frame* frames, int n_frames, double* out_coords, double* out_angles,
                                        int32_t* out_orig_index, double* out_confidence, int64_t out_cap, int32_t* frame_first,
                                        int32_t* stage_counts, int64_t* rows_executed, void* stream);
/* hg_cascade_detect_faces_frames_device for a list: the pooled stage loop above, the eye step on ALL survivors as one batch, every eye
 * patch cut from its face's own prescaled frame, the purge per frame.  Outputs and refusals as there and as above.  Synchronous. */
int hg_cascade_detect_faces_frame_list_device(hg_cascade* c, hg_eyes* e, const hg_cascade_frame* frames, int n_frames, double* out_rows,
                                              int64_t out_cap, int32_t* frame_first, int32_t* n_before_purge, int32_t* stage_counts,
                                              int64_t* rows_executed, void* stream);

/* --- Tracking one face across a stream of frames (the reference's track_single_face mode) ---------------------------------
 * Once a frame has produced a face, its first purged detection is carried over (FaceDetectUpdated.py:1189-1195) and the next
 * frame searches NINE windows instead of the pyramid: one sampling value from the size of that box (face_analysis.py:576-585),
 * the box's corner and one horizontal separation step to either side, all at the box's own y (:611-623); the product of the two
 * position lists (:661-669) is the three distinct windows three times over, y-major, and the duplicates reach the purge as in the
 * reference.  A tracked frame that finds nothing sends the following frame back to the full grid.
 *   sampling  = (0.5 |x1 - x0| + 0.5 |y1 - y0|) * 1.0 / subimage_width
 *   patch     = (subimage_width * sampling, subimage_height * sampling)
 *   sepx      = net_Dx * 2.0 * patch_w / regression_width;   posX = (x0, x0 + sepx, x0 - sepx), posY = (y0, y0, y0)
 *   window    = (posX, posY, posX + patch_w - 1, posY + patch_h - 1)
 *   level     = (net_Dx * patch_w / regression_width, net_Dy * patch_h / regression_height, sqrt(patch_w^2 + patch_h^2))
 * float64 in that operation order, no contraction: bit for bit the reference's (tests/golden/reference_tracking.npz). */
typedef struct hg_tracked_consts {
    double subimage_width, subimage_height;      /* the cascade's sub-image size                              */
    double regression_width, regression_height;  /* Pipeline header: 128 128                                  */
    double net_Dx, net_Dy;                       /* Pipeline header: 40 20                                    */
} hg_tracked_consts;
/* The nine windows alone, for inspection: face_dev (4 doubles ON THE DEVICE: x0, y0, x1, y1) -> boxes_dev (9, 4) and level_dev (9, 3),
 * float64 on the device.  Enqueued on `stream`. */
int hg_cascade_tracked_grid_device(int device, const hg_tracked_consts* consts, const double* face_dev, double* boxes_dev, double* level_dev,
                                   void* stream);
/* The same for n_faces boxes in one launch (the grid kernel of a tracker that holds several faces): faces_dev (n_faces, 4) float64 ON THE
 * DEVICE -> boxes_dev (9 * n_faces, 4) and level_dev (9 * n_faces, 3); window 9 s + i is window i of face s, the bits the single form
 * writes for that face.  HG_ERR_ARG for a null pointer, n_faces < 1 and constants that are not positive and finite. */
int hg_cascade_tracked_grid_multi_device(int device, const hg_tracked_consts* consts, const double* faces_dev, int n_faces, double* boxes_dev,
                                         double* level_dev, void* stream);
/* The tracker: created from a cascade and an eye handle on one device (both stay owned by the caller and must outlive it; consts'
 * sub-image size must be the cascade's).  It owns, on the device, the tracked box and its found flag, and remembers the size of the
 * prescaled frame the box belongs to.
 * hg_tracker_step_frame_device takes the arguments of hg_cascade_detect_faces_frame_device and returns the same rows.
 *   - No face held, or the prescaled frame size differs from the one the face was found at: exactly what
 *     hg_cascade_detect_faces_frame_device runs (*used_tracked_grid = 0); then row 0's box, if there is a row, becomes the tracked
 *     face.  A change of the prescaled size DROPS the tracked face — its coordinates mean nothing on another size; the reference
 *     has no such case (it applies the box to whatever frame comes next).
 *   - Otherwise the tracked frame (*used_tracked_grid = 1): the nine windows are built on the device from the box the previous
 *     frame's purge left there, and the whole frame — grid, every stage group, eyes, purge, hand-over of the new tracked face — is
 *     enqueued back to back.  Every launch is sized by the bound 9 (the eye launches by 18); the kernels take the live count from
 *     device memory; rows between the live count and the bound are given a defined window.  No survivor count is read back:
 *     stage_counts[] is -1 throughout, and the call ends with ONE host wait that fetches the kept count, the rows and the flag.
 *     `levels` is not read.  *rows_executed counts 9 rows per network-owning stage.
 * The box is carried only if its four numbers are finite.  The box is in the coordinates of the prescaled frame the cascade read and
 * is applied to the next prescaled frame, as in the reference.  One stream per handle, as for the patcher: a step must not run
 * while another step of the same tracker, or any call on its cascade or eye handle, is in flight; one frame at a time.
 * hg_tracker_reset forgets the face (the next step uses the full grid).  Synchronous. */
typedef struct hg_tracker hg_tracker;
int hg_tracker_create(hg_cascade* c, hg_eyes* e, const hg_tracked_consts* consts, hg_tracker** out);
void hg_tracker_free(hg_tracker* t);
int hg_tracker_reset(hg_tracker* t);
int hg_tracker_step_frame_device(hg_tracker* t, const void* frame_dev, int frame_h, int frame_w, int64_t ld, int prescale_w, int prescale_h,
                                 const hg_cascade_level* levels, int n_levels, double* out_rows, int64_t out_cap, int64_t* n_out,
                                 int64_t* n_before_purge, int32_t* stage_counts, int64_t* rows_executed, int* used_tracked_grid, void* stream);

/* --- Several tracked faces ------------------------------------------------------------------------------------------------
 * hg_tracker_create_multi: a tracker that holds up to max_faces faces (1..64) and, with rescan_every = R > 0, returns to the full grid
 * after R consecutive tracked steps (0: never, as the reference).  hg_tracker_create is (max_faces, rescan_every) = (1, 0).  HG_ERR_ARG
 * for max_faces outside 1..64 and for rescan_every < 0, before any handle is looked at.
 * The path of a step is decided on the host.  A FULL-GRID step when nothing is held, when the prescaled size differs from the one the
 * boxes belong to (all held boxes are dropped), or when R > 0 and R tracked steps have run since the last full-grid step: exactly
 * hg_cascade_detect_faces_frame_device's work, then the hand-over.  Otherwise a TRACKED step with K = the held count: window 9 s + i is
 * window i of held face s, the whole frame runs under the bound 9 K (the eye launches under 18 K) as described above with 9 K in the
 * place of 9, the purge runs over the union of all faces' rows, *rows_executed counts 9 K rows per network-owning stage.
 * The hand-over (both paths): candidates are the first min(kept, max_faces) purged rows; those whose four box numbers are all finite are
 * carried, in purge order, as the held faces of the next step.  *n_held (nullable): that count.
 * slots (nullable, out_cap entries): slots[j] is the index, in the previous step's carried order, of the held face whose nine windows
 * produced kept row j; when the purge appends its first row a second time both copies carry the same slot; -1 for every row of a
 * full-grid step.
 * HG_ERR_ARG, writing no row and no slot, when out_cap is below the kept count (the hand-over has happened by then: *n_held is valid).
 * hg_tracker_step_frame_device on such a handle is this call with slots = n_held = NULL.  One stream per handle, as above: a step must
 * not run while another step of the same tracker, or any call on its cascade or eye handle, is in flight.  Synchronous. */
int hg_tracker_create_multi(hg_cascade* c, hg_eyes* e, const hg_tracked_consts* consts, int max_faces, int rescan_every, hg_tracker** out);
int hg_tracker_step_frame_multi_device(hg_tracker* t, const void* frame_dev, int frame_h, int frame_w, int64_t ld, int prescale_w, int prescale_h,
                                       const hg_cascade_level* levels, int n_levels, double* out_rows, int64_t out_cap, int64_t* n_out,
                                       int64_t* n_before_purge, int32_t* stage_counts, int64_t* rows_executed, int* used_tracked_grid,
                                       int32_t* slots, int* n_held, void* stream);

/* --- Tracking faces on a SET of frame streams in one pooled step ----------------------------------------------------------------
 * hg_stream_tracker: n_streams trackers in one handle.  Stream s behaves exactly as an hg_tracker_create_multi(c, e, consts, max_faces,
 * rescan_every) of its own that is fed frame s of every stack, step after step: the same boxes in the same carried order, the same
 * path rule (FULL GRID when the stream holds nothing or, with rescan_every = R > 0, after R tracked steps in a row, counted per stream;
 * TRACKED otherwise), the same hand-over rule, and a change of the prescaled size drops the boxes of EVERY stream.
 * hg_stream_tracker_create: HG_ERR_ARG, the numbers before any handle is looked at, for n_streams outside 1..HG_MAX_STACK_FRAMES,
 * max_faces outside 1..64, 9 n_streams max_faces above HG_MAX_STREAM_WINDOWS, rescan_every < 0; then as hg_tracker_create_multi.
 *   HG_MAX_STREAM_WINDOWS = 8192: the tracked pass runs under a bound and relies on the filler rows the stage loop's single-workgroup
 *   glue kernel writes between the live count and the bound; above 8192 candidates the stage loop takes its chunked two-launch glue,
 *   which writes none.
 * hg_stream_tracker_reset(t, s): stream s forgets its faces (its next step uses the full grid); s = -1: every stream.  HG_ERR_ARG for
 * another s.  Synchronous.
 * hg_stream_tracker_step_frames_device: one frame per stream.  The frame arguments are hg_cascade_detect_faces_frames_device's
 * (frame 0, n_frames, frame_stride, frame_h, frame_w, ld in the cascade's frame format, the prescale size, the levels of the full
 * grid, which are checked on every step).  With T = the streams on the tracked path and G = the others:
 *   1. the tracked pass, enqueued whole: one kernel builds the nine windows of every held face of every stream of T from the state on
 *      the device (hg_cascade_tracked_grid_streams_device is that kernel alone); the stage loop runs under the bound 9 * (faces held in
 *      T), known on the host, every extraction cutting a row from its own stream's frame; the eye step runs on all survivors as one
 *      batch (18 * ... rows), the purge per stream; a hand-over kernel, one workgroup per stream, writes the stream's carried boxes and
 *      count into the state and its kept rows, counts and slots to pinned memory; a sequence word follows behind it.  No count is read
 *      back.
 *   2. the full-grid pass: what hg_cascade_detect_faces_frames_device runs on the frames of G (copied together unless they are all
 *      the frames, one frame, or prescaled / converted anyway), then the hand-over of every stream's first rows.
 *   3. the one wait of the tracked pass.
 * A pass without streams launches nothing.  Outputs (host; all but stream_first nullable): out_rows, the kept rows ordered by stream,
 * stream s's at stream_first[s] .. stream_first[s + 1] (n_streams + 1 entries); slots (out_cap entries), per row as
 * hg_tracker_step_frame_multi_device's, relative to the stream's carried order, -1 on a full-grid step; per stream n_before_purge,
 * used_tracked_grid (0 / 1) and n_held; *rows_executed, the rows of both passes (9 * faces held in T per network-owning stage, plus
 * the full-grid pass's).  Per-stage survivor counts are not offered: the pooled passes do not have them per stream.
 * HG_ERR_ARG before anything is launched or written — the numbers before the handle: n_frames outside 1..HG_MAX_STACK_FRAMES, a bad
 * frame geometry, frame_stride below (frame_h - 1) ld + frame_w bytes-per-pixel, out_cap < 0; then a null handle or stream_first,
 * n_frames != n_streams, and hg_cascade_detect_faces_frames_device's other refusals.  HG_ERR_ARG, writing no row and no slot
 * (stream_first all 0), when out_cap is below the kept total: the hand-overs have happened by then and n_held is valid.  After any
 * other failure every stream holds nothing.  One stream per handle, as above: a step must not run while another step of the set, or any
 * call on its cascade or eye handle, is in flight.  Synchronous. */
#define HG_MAX_STREAM_WINDOWS 8192
typedef struct hg_stream_tracker hg_stream_tracker;
int hg_stream_tracker_create(hg_cascade* c, hg_eyes* e, const hg_tracked_consts* consts, int n_streams, int max_faces, int rescan_every,
                             hg_stream_tracker** out);
void hg_stream_tracker_free(hg_stream_tracker* t);
int hg_stream_tracker_reset(hg_stream_tracker* t, int stream_index);
int hg_stream_tracker_step_frames_device(hg_stream_tracker* t, const void* frames_dev, int n_frames, int64_t frame_stride, int frame_h,
                                         int frame_w, int64_t ld, int prescale_w, int prescale_h, const hg_cascade_level* levels,
                                         int n_levels, double* out_rows, int64_t out_cap, int32_t* stream_first, int32_t* n_before_purge,
                                         int32_t* used_tracked_grid, int32_t* n_held, int32_t* slots, int64_t* rows_executed, void* stream);
/* The grid kernel of the tracked pass alone, for inspection: faces_dev (n_streams, max_faces, 4) float64 and held_dev (n_streams) int32
 * ON THE DEVICE -> boxes_dev (9 n_streams max_faces, 4) and level_dev (.., 3): window s * 9 max_faces + 9 j + i is window i of held
 * face j < held[s] of stream s, the bits hg_cascade_tracked_grid_multi_device writes for that face; the rows of faces not held are
 * not written.  A count outside 0..max_faces is read as the nearer end.  HG_ERR_ARG for n_streams outside 1..HG_MAX_STACK_FRAMES,
 * max_faces outside 1..64, a null pointer, constants that are not positive and finite.  Enqueued on `stream`. */
int hg_cascade_tracked_grid_streams_device(int device, const hg_tracked_consts* consts, const double* faces_dev, const int32_t* held_dev,
                                           int n_streams, int max_faces, double* boxes_dev, double* level_dev, void* stream);

/* --- SFA training step for one layer of nodes (BASELINE.json configs[4]) -----
 * Not on the reference's path (it never trains, face_analysis.py:451-479); restates
 * mdp.nodes.SFANode train/stop_training per node k over input columns conn[k*d .. (k+1)*d):
 * mean, B = Cov(x), A = Cov(x[t+1]-x[t]) accumulated in fp64 by a HIP kernel, then
 * A w = lambda B w (eigenvalues ascending, w' B w = 1): hand-written Jacobi kernel for d <= 16, rocSOLVER dsygvj
 * for wider nodes (HIGSFA_SYGVJ=1 / HIGSFA_SYGVD=1 force rocSOLVER's dsygvj / dsygvd).
 * x: (n, ldx) matrix in time order, a device pointer or (x_on_host != 0) a host pointer that is
 * copied to the device first.  Host outputs: evals (n_nodes, d), evecs
 * (n_nodes, d, d) column-major per node (column i = eigenvector i), mean (n_nodes, d);
 * timings_ms[2] (optional): statistics kernels, solve.
 * Refusals: HG_ERR_ARG for n < 3, d outside 1..128, an unknown dtype, a null pointer, a column outside [0, ldx);
 * HG_ERR_STATE naming the first node whose B is not positive definite (a constant column; a column listed twice
 * in one node, refused before the solve; for d <= 16 a NaN in the input) or whose Jacobi sweeps did not converge
 * (info = 17 from the hand-written solver). */
int hg_sfa_train_layer(const void* x, int x_on_host, int x_dtype, int64_t n, int64_t ldx, const int32_t* conn_host,
                       int32_t n_nodes, int32_t d, int device, double* evals_host, double* evecs_host,
                       double* mean_host, double* timings_ms);
/* The PCA / whitening step of a node (mdp.nodes.PCANode / WhiteningNode train + stop_training): same statistics kernel, then the
 * eigen-decomposition of Cov(x) itself (the same solver on (Cov, I)): evals ascending, orthonormal eigenvectors.  A singular
 * covariance (n <= d, a constant column, a column listed twice) is legal here; for d <= 16 a NaN in the input is HG_ERR_STATE (the sweeps cannot converge). */
int hg_pca_train_layer(const void* x, int x_on_host, int x_dtype, int64_t n, int64_t ldx, const int32_t* conn_host,
                       int32_t n_nodes, int32_t d, int device, double* evals_host, double* evecs_host,
                       double* mean_host, double* timings_ms);
/* What a trained step passes on during training, in float64 like MDP: out[t, node * width + f * p + j] =
 * func_f(((x[t, conn[node]] - mean[node]) W[node])_j), width = max(1, n_funcs) * p; n_funcs = 0: the affine map alone.
 * func_kinds: 0 identity, 1 |z|^e, 2 sgn(z)|z|^e.  x_dev / out_dev: device; conn / mean / W (n_nodes, d, p row-major): host. */
int hg_train_apply_device(const void* x_dev, int x_dtype, int64_t n, int64_t ldx, const int32_t* conn_host, int32_t n_nodes,
                          int32_t d, const double* mean_host, const double* w_host, int32_t p, int32_t n_funcs,
                          const int32_t* func_kinds, const double* func_expos, double* out_dev, int64_t ldo, int device);

/* --- Age, race and gender estimation (estimate_age_race_gender, face_analysis.py:1170-1306; FaceDetectUpdated.py:1186-1187) ----------
 * Per purged face: the pose-normalised crop (hg_patcher_normalize_device with crop_w x crop_h, method, rotate), ONE patch_w x patch_h
 * sub-image of it with the contrast step, the age network (networks[num_networks - 3]; the Race and Gender stages have no network and
 * reuse its features, Pipelines/Pipeline_experimental.txt:62-70), and up to three regressions on the same features: age with its std,
 * race, gender.  The sub-image is cut by cuicuilco's load_image_data_monoprocessor, which is not available; the three rules are the
 * build's, tested against PIL:
 *   box       in crop coordinates, a plain parameter (pyfaceanalysis_amd.analysis.age_patch_box evaluates the reference's visible
 *             expressions, :1182-1197: about (36.8, 31.96, 219.2, 214.36) for the reference's constants)
 *   cut       crop.transform((patch_w, patch_h), EXTENT, box, filter): the rule of hg_patcher_extract_filter_device without rotation;
 *             a box partly outside the crop reads zeros there
 *   contrast  the eye step's: S1 = sum p, S2 = sum p^2 as int64 over the N patch pixels (the zeros included), mean = S1 / N,
 *             std = sqrt((N S2 - S1^2) / (N N)), p' = (p - mean) / (std / target_std + 1e-8) + target_mean as float32; clip = 1 clips
 *             p' to [0, 255] first (face_analysis.py:327, the only rule the reference shows), clip = 0 does not (the reference's
 *             obj_avgs = 0.0 makes sense only unclipped).  The targets are required.
 * Patches of at most 16384 pixels can go through one fused kernel (cut + contrast, one workgroup per face); larger ones, and any patch
 * with flag bit 0, go through hg_patcher_extract_filter_device per face and a contrast kernel.  Same bits either way.  The default is
 * the fused kernel where it measured faster (every case but BICUBIC with fewer than four faces; profiles/r16_analysis_times.txt). */
typedef struct hg_estimator hg_estimator;
typedef struct hg_estimator_consts {
    int32_t crop_w, crop_h, method, rotate;   /* as hg_norm_consts: 256, 260, HG_NORM_AREAZ, 1                      */
    int32_t patch_w, patch_h;                 /* 96 x 96; at most 4096 per side and 65536 pixels                    */
    int32_t filter;                           /* enum hg_filter                                                     */
    int32_t clip;                             /* 1 / 0                                                              */
    double  box[4];                           /* x0, y0, x1, y1 in crop coordinates, finite                         */
    double  target_mean, target_std;          /* required; target_std > 0                                           */
    int32_t n_features, reserved;             /* feature columns kept (>= every classifier's input_dim); 0          */
} hg_estimator_consts;
/* Any of age / race / gender may be null (that estimate is not computed), not all three.  The flow's input width is patch_w * patch_h
 * and it gives at least n_features columns; every classifier's input_dim is <= n_features.  The flow and the patcher live on `device`
 * (the classifiers too).  HG_ERR_ARG / HG_ERR_DIM on a violation, checked in this order: constants, the flow's shape, the classifiers,
 * the devices.  All handles stay owned by the caller and must outlive the estimator. */
int hg_estimator_create(hg_flow* flow, hg_gauss* age, hg_gauss* race, hg_gauss* gender, const hg_estimator_consts* consts, hg_patcher* patcher,
                        int device, hg_estimator** out);
void hg_estimator_free(hg_estimator* e);
/* The patch step alone: crops_dev n uint8 images of crop_h x crop_w, crop_stride >= crop_w * crop_h bytes apart -> patches_dev n rows of
 * patch_w * patch_h float32, ldp >= that many floats apart.  flags: bit 0 forces the composed path, bit 1 the fused kernel (HG_ERR_ARG
 * above 16384 pixels; not both); other bits HG_ERR_ARG.  Enqueued on `stream`. */
int hg_estimator_patches_device(hg_estimator* e, int flags, const uint8_t* crops_dev, int64_t crop_stride, int64_t n, float* patches_dev, int64_t ldp,
                                void* stream);
/* The whole chain for the n faces of geoms_host (hg_normalize_geometry_host for this frame size and the estimator's crop constants;
 * consumed before the call returns) on frame_dev ((frame_h, frame_w) grey uint8, rows ld bytes apart): normalise into the estimator's
 * crop scratch, patches, hg_flow_execute_device (float32, n_features columns), age through hg_gauss_regression_device with its std, race
 * and gender through hg_gauss_regression_multi_device, a finishing kernel.  Enqueued on `stream`; the host is not waited for.
 * out_dev: (4, n) float64, rows out_stride >= n apart: age, age_std, race, gender.  The rows of an absent classifier hold the reference's
 * initial values 0, 0, 10, 10 (face_analysis.py:1201-1204).  A refused face (geoms_host[i].status != 0) has NaN in all four rows; no
 * other face's bits depend on it.  patches_dev (n, patch_w * patch_h) / features_dev (n, n_features), float32, contiguous, nullable:
 * the intermediates.  flags as above.  Scratch (crops, patches, features, refused flags) grows on demand, and growing waits for `stream`;
 * ONE STREAM PER ESTIMATOR, the patcher's rule (the patcher, the flow and the classifiers must not be in use elsewhere meanwhile).
 * n == 0: HG_OK, nothing launched. */
int hg_estimator_estimate_device(hg_estimator* e, int flags, const uint8_t* frame_dev, int frame_h, int frame_w, int64_t ld,
                                 const hg_norm_geom* geoms_host, int64_t n, double* out_dev, int64_t out_stride, float* patches_dev,
                                 float* features_dev, void* stream);

/* --- Pose normalisation and estimation over a stack of same-size frames (the rows of hg_cascade_detect_faces_frames_device) ----------
 * Every step of the chain above is independent per face, so each result below is DEFINED as what the single-frame entry returns for
 * that face on its own frame, bit for bit (tests/test_estimate_frames_gpu.py).
 *
 * hg_patcher_normalize_device for n faces spread over a stack: face i is cut from frame face_frame_host[i] (host, int32, consumed before
 * the call returns) of n_frames grey uint8 frames, all frame_h x frame_w with row stride ld, frame f starting frame_stride BYTES behind
 * frame f - 1 — any value >= (frame_h - 1) ld + frame_w, not necessarily a multiple of ld, as for hg_patcher_extract_frames_device.
 * The geoms are those of hg_normalize_geometry_host for the one frame size.  A pixel of the virtual crop is
 * frames_dev[index * frame_stride + fy * ld + fx] inside that frame and 0 outside it, all offsets 64-bit.  A face whose index lies
 * outside [0, n_frames) is treated like a refused face — an all-zero image, no address formed from the index — and is NOT an error.
 * Staged and tap by tap as above (the same flags, the same bytes); the face records and the scratch are the patcher's, sized from the
 * host geoms alone.  The single-frame entry runs its own kernel instantiations with the records it has always had.
 * HG_ERR_ARG before the device is touched and without reading anything behind frames_dev / out_dev: everything the single-frame entry
 * refuses, n_frames < 1 or > HG_MAX_STACK_FRAMES, frame_stride below the bound, a null face_frame_host with n > 0.  n == 0: HG_OK,
 * nothing launched. */
int hg_patcher_normalize_frames_device(hg_patcher* p, int flags, const uint8_t* frames_dev, int n_frames, int64_t frame_stride, int frame_h,
                                       int frame_w, int64_t ld, const hg_norm_geom* geoms_host, const int32_t* face_frame_host, int64_t n,
                                       int out_w, int out_h, uint8_t* out_dev, int64_t ldo, void* stream);
/* hg_estimator_estimate_device on the pooled faces of a stack: ONE normalise (the entry above) into the estimator's crop scratch, one
 * patch step, one hg_flow_execute_device on n rows, the regressions on n rows, the finishing kernel.  out_dev, patches_dev,
 * features_dev, flags, the scratch and the one-stream rule as there.  A face whose frame index lies outside [0, n_frames) has NaN in all
 * four rows, as a refused face has; no other face's bits depend on it.  Refusals (HG_ERR_ARG, nothing launched; all but the fused
 * kernel's pixel cap are decided without reading the handle): those of the entry above about the stack, the geoms and face_frame_host,
 * out_stride < n, a null out_dev with n > 0, n above 2^20, bad flags.  n == 0: HG_OK, nothing launched.
 * The prescaled grey stack these coordinates refer to is composed in Python (DeviceCascade.prescale_frames: the per-frame prescale
 * into the slices of one tensor); there is no C entry for it. */
int hg_estimator_estimate_frames_device(hg_estimator* e, int flags, const uint8_t* frames_dev, int n_frames, int64_t frame_stride, int frame_h,
                                        int frame_w, int64_t ld, const hg_norm_geom* geoms_host, const int32_t* face_frame_host, int64_t n,
                                        double* out_dev, int64_t out_stride, float* patches_dev, float* features_dev, void* stream);

/* --- Pose normalisation and estimation over a LIST of frames of different sizes (the rows of hg_cascade_detect_faces_frame_list_device) --
 * The two entries above for a list: face i is cut from frames[face_frame_host[i]], a grey uint8 frame with its OWN pointer, size and row
 * stride (hg_frame_ref, ld in BYTES; the descriptor array is host memory, consumed before the call returns).  Each result is DEFINED as
 * what the single-frame entry returns for that face on its own frame, bit for bit (tests/test_estimate_frame_list_gpu.py).
 * geoms_host[i] MUST HAVE BEEN COMPUTED FOR THE SIZE OF FACE i's OWN FRAME (hg_normalize_geometry_host with frames[face_frame_host[i]]'s
 * frame_w, frame_h): a geom built for another size is refused.  The host resolves every face's frame into its record — one upload per
 * call, as for the stack; no table of frames on the device.  A face whose index lies outside [0, n_frames) is treated like a refused
 * face — an all-zero image, no address formed, its geom not looked at — and is NOT an error.  Staged and tap by tap, the flags, the
 * 2^24 face bound, the records and the scratch as above; every grid and scratch size comes from the host geoms.  Frames of ONE size stay
 * the stack entries' case.  Enqueued on `stream`; the host is not waited for.
 * HG_ERR_ARG before anything is launched or written, reading nothing behind a frame pointer or out_dev: what the stack entry refuses about
 * n, the flags, the output size and ldo, a null geoms_host / face_frame_host / out_dev with n > 0, n_frames < 1 or > HG_MAX_STACK_FRAMES,
 * a null frames, ANY frame with frame_h <= 0, frame_w <= 0, ld < frame_w, a null frame_dev or more than 2^24 pixels per side — the
 * message names the frame, and one bad frame refuses the whole call.  n == 0: HG_OK, nothing launched. */
int hg_patcher_normalize_frame_list_device(hg_patcher* p, int flags, const hg_frame_ref* frames, int n_frames, const hg_norm_geom* geoms_host,
                                           const int32_t* face_frame_host, int64_t n, int out_w, int out_h, uint8_t* out_dev, int64_t ldo,
                                           void* stream);
/* hg_estimator_estimate_frames_device on the pooled faces of a list: the same chain on the same rows with the normalise entry above in
 * front — one normalise, one patch step, one hg_flow_execute_device, the regressions, the finishing kernel.  out_dev ((4, n) float64,
 * rows ldo >= n apart), patches_dev, features_dev, flags, the scratch and the one-stream rule as there.  A face whose frame index lies
 * outside [0, n_frames) has NaN in all four rows.  Refusals: those of the entry above about the list, the geoms and face_frame_host,
 * ldo < n, a null out_dev with n > 0, n above 2^20, bad flags.  n == 0: HG_OK, nothing launched.  The prescaled grey frames the rows of the
 * cascade's list entries refer to are composed in Python (DeviceCascade.prescale_frame_list); there is no C entry for them. */
int hg_estimator_estimate_frame_list_device(hg_estimator* e, int flags, const hg_frame_ref* frames, int n_frames, const hg_norm_geom* geoms_host,
                                            const int32_t* face_frame_host, int64_t n, double* out_dev, int64_t ldo, float* patches_dev,
                                            float* features_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HIGSFA_H */
