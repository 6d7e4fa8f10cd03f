/* libocrvi -- C ABI of the MI355X-native (gfx950) DBNet++ / SVTRv2 / CTC inference hot path.
 *
 * The reference (ZenHKD/ocr-vi-invoice) is pure Python and has no FFI; the hot path sits behind two
 * torch.nn.Module forward APIs.  Each entry point below names the reference interface it replaces.
 * Plain pointers and sizes only -- no torch types.  All device pointers are HIP device memory on the
 * handle's device.  Every *_forward only enqueues work on `stream` (a hipStream_t passed as void*): no
 * allocation, no host synchronisation, so calls are graph-capturable.  The caller owns inputs, outputs
 * and workspace; a handle owns its (repacked) weights only.  Handles are per-device and not thread-safe.
 *
 * Errors: every function returns 0 (OCRVI_OK) or a negative code and never aborts the process;
 * ocrvi_last_error() returns a thread-local message for the last failing call.
 */
#ifndef OCRVI_H
#define OCRVI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OCRVI_OK 0
#define OCRVI_EINVAL (-1) /* bad shape / alignment / argument (reference: ATen shape errors, svtrv2.py:425 assert) */
#define OCRVI_EHIP (-2)   /* a HIP runtime call failed; message carries hipGetErrorString */
#define OCRVI_ENOMEM (-3) /* workspace too small */
#define OCRVI_EBLOB (-4)  /* weight blob malformed or a tensor is missing / has the wrong shape */
#define OCRVI_ERANGE (-5) /* OCRVI_F16X2 only: an intermediate activation left fp16's exponent range (|x| >= 65520); reference: none -- the
                             reference is fp32 end to end (src/pipeline/pipeline2.py:312-318), so this mode says when it cannot stand in for it */

/* Arithmetic type the MFMA kernels compute in (accumulation is always fp32).
 * OCRVI_F32   fp32 operands on v_mfma_f32_16x16x4_f32: bit for bit an fp32 fmaf chain (what the reference's CPU path computes in).
 * OCRVI_F16X2 fp32-equivalent operands on the 16-bit matrix pipe: every GEMM operand element is stored as two fp16 halves
 *             x = hi + lo (>= 22 significant bits, weights scaled by a power of two per layer) and every product is formed from the
 *             three partial products hi hi + hi lo + lo hi in fp32 accumulators (the lo lo term, <= 2^-22 of a product, is dropped;
 *             conv_gemm's 64- and 32-column tiles compute all four); same API, same fp32 inputs and outputs.
 *             Supported activation range: fp16's exponent.  An intermediate activation with |x| >= 65520 cannot be represented
 *             (its hi half would be infinite): every kernel that writes f16x2 elements raises the handle's overflow flag instead of
 *             passing it on silently, and ocrvi_det_status / ocrvi_rec_status report it (below).  Below |x| = 2^-3 the absolute error
 *             of an element is 2^-25 (its lo half is a subnormal fp16 number), so tensors whose rms is under about 2^-9 lose the
 *             fp32-equivalence (relative error 2^-25 / |x|): BatchNorm / LayerNorm keep the two models' activations at O(0.1 .. 10).
 * OCRVI_BF16 / OCRVI_F16  plain 16-bit operands (throughput modes). */
typedef enum { OCRVI_F32 = 0, OCRVI_BF16 = 1, OCRVI_F16 = 2, OCRVI_F16X2 = 3 } ocrvi_dtype;

const char* ocrvi_last_error(void);
/* ABI version of this header (bumped on any signature change). */
int ocrvi_abi_version(void);

/* ------------------------------------------------------------------------------------------------
 * Detection: replaces DBNetPP(backbone in {'resnet50', 'resnet18'}, dcn in {True, False}).eval() -- model/det/dbnet.py:6-17
 * (ResNet-50 or ResNet-18 backbone model/det/backbone.py:8-60, the choice at backbone.py:12-15, torchvision's Bottleneck /
 * BasicBlock; with dcn every block's conv2 in layers 2-4 is the DCNv2 module, backbone.py:28-31,39-53, dcn.py:41-59; FPN+ASF neck
 * neck.py:26-79; DB head head.py:32-48).
 * ------------------------------------------------------------------------------------------------ */
typedef struct ocrvi_det ocrvi_det;

typedef struct {
    int32_t dtype;   /* ocrvi_dtype */
    float k;         /* DB step-function steepness, head.py:6,28-30 (reference default 50) */
    int32_t max_batch;  /* largest N a forward call will see (sizes nothing; validated only) */
    int32_t backbone;   /* 0 = ResNet-50 (Bottleneck [3,4,6,3]), 1 = ResNet-18 (BasicBlock [2,2,2,2]) -- backbone.py:12-15; else OCRVI_EINVAL */
    int32_t no_dcn;     /* 0 = DeformableConv2d as conv2 of every block of layer2..4 (backbone.py:28-31), 1 = plain 3x3; else OCRVI_EINVAL */
    int32_t reserved[3];   /* a zeroed struct is ResNet-50 with DCN; the blob must be of the same architecture (OCRVI_EINVAL otherwise) */
} ocrvi_det_cfg;

/* `blob` = host bytes produced by ocr_vi_invoice_amd.weights.pack_blob(fold_det(state_dict)): BN already
 * folded (eval-mode running stats), standard OIHW fp32 tensors.  Replaces load_state_dict + .to(device) +
 * .eval() of load_detection_model (src/pipeline/pipeline2.py:43-54). */
int ocrvi_det_create(int device, const void* blob, size_t blob_bytes, const ocrvi_det_cfg* cfg, ocrvi_det** out);
void ocrvi_det_destroy(ocrvi_det* h);
/* Bytes of scratch device memory one forward of shape (N,3,H,W) needs. */
int ocrvi_det_workspace_bytes(const ocrvi_det* h, int N, int H, int W, size_t* bytes);
/* Replaces DBNetPP.forward (dbnet.py:13-17).  x: float32 NCHW [N,3,H,W], H and W multiples of 32
 * (pipeline2.py:33-40 guarantees it).  Outputs are float32 [N,1,H,W]; `binary` is required, the other four
 * dict entries of head.py:42-48 may be NULL (then not written; the arithmetic that produces them is still
 * the same two-branch head: a caller that reads `binary` alone wants ocrvi_det_forward_binary below). */
int ocrvi_det_forward(ocrvi_det* h, const float* x, int N, int H, int W,
                      float* binary, float* thresh, float* thresh_binary, float* bin_logits, float* thresh_logits,
                      void* workspace, size_t workspace_bytes, void* stream);
/* Replaces DBNetPP.forward as the page loop uses it: `pred_binary = preds['binary']` is the one map inference reads
 * (src/pipeline/pipeline2.py:318); thresh, thresh_binary and the two logit maps exist for the training loss.  Backbone, FPN and ASF as in
 * ocrvi_det_forward; of the head only the binarise branch runs (head.py:34: ConvBnRelu(256,64,3), two ConvTranspose2d, Sigmoid -- the
 * threshold branch, head.py:38, about 8 % of the forward's FLOPs, is not computed), the sigmoid sits in the last deconvolution's epilogue
 * and no logit map is written.  binary: float32 [N,1,H,W], bit for bit the `binary` of ocrvi_det_forward on the same handle and input in
 * the OCRVI_F32 and OCRVI_F16X2 modes (the branch runs on views of the same packed weights).  Same contract otherwise: shape rules,
 * 256-byte aligned workspace of ocrvi_det_binary_workspace_bytes (never more than ocrvi_det_workspace_bytes), OCRVI_ENOMEM when it is
 * short, enqueue-only on `stream`, graph-capturable, range flag snapshot for ocrvi_det_status. */
int ocrvi_det_binary_workspace_bytes(const ocrvi_det* h, int N, int H, int W, size_t* bytes);
int ocrvi_det_forward_binary(ocrvi_det* h, const float* x, int N, int H, int W, float* binary,
                             void* workspace, size_t workspace_bytes, void* stream);
/* Test hook: copies of intermediate features as float32 NCHW (c2..c5 backbone.py:56-60, fused neck.py:79).
 * c2..c5 have 256 / 512 / 1024 / 2048 channels for ResNet-50 and 64 / 128 / 256 / 512 for ResNet-18, at H/4 .. H/32; fused has 256 at H/4.
 * Any pointer may be NULL.  Must follow a forward on the same workspace and stream. */
/* OCRVI_F16X2 handles: OCRVI_OK, or OCRVI_ERANGE when an f16x2 kernel on this handle's device has met a value fp16's exponent cannot
 * carry since the last ocrvi_range_reset (the flag is per device and sticky; *_forward copies it to the handle asynchronously on the
 * caller's stream, so call this AFTER synchronising that stream -- never a host sync inside *_forward).  Other dtypes: always OCRVI_OK. */
int ocrvi_det_status(const ocrvi_det* h);
int ocrvi_det_debug_features(ocrvi_det* h, int N, int H, int W, float* c2, float* c3, float* c4, float* c5,
                             float* fused, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Recognition: replaces SVTRv2(variant).eval() -- model/rec2/svtrv2.py:410-569 (inference graph; the
 * SGM branch, svtrv2.py:252-385, is training-only and not built).
 * ------------------------------------------------------------------------------------------------ */
typedef struct ocrvi_rec ocrvi_rec;

typedef struct {
    int32_t dtype;        /* ocrvi_dtype */
    int32_t dims[3];      /* VARIANTS[..]['dims']       svtrv2.py:391-407 */
    int32_t num_blocks[3];/* VARIANTS[..]['num_blocks'] */
    int32_t num_local[3]; /* VARIANTS[..]['num_local']  (first num_local blocks of a stage are LocalMixing) */
    int32_t num_classes;  /* tokenizer.num_classes = 232 (tokenizer.py:21) */
    int32_t blank_id;     /* 0 (tokenizer.py:14) */
    int32_t reserved[4];
} ocrvi_rec_cfg;

/* `blob` = pack_blob(fold_rec(state_dict, variant)).  Replaces load_recognition_model
 * (src/pipeline/pipeline2.py:72-82). */
int ocrvi_rec_create(int device, const void* blob, size_t blob_bytes, const ocrvi_rec_cfg* cfg, ocrvi_rec** out);
void ocrvi_rec_destroy(ocrvi_rec* h);
int ocrvi_rec_workspace_bytes(const ocrvi_rec* h, int B, int H, int W, size_t* bytes);
/* Replaces SVTRv2.forward(x, targets=None) (svtrv2.py:503-536) fused with decode_probs' device half
 * (svtrv2.py:555-566).  x: float32 NCHW [B,3,H,W], H % 16 == 0 and W % 4 == 0, T = W/4.
 *   log_probs [T,B,num_classes] float32 (may be NULL)
 *   argmax_ids [B,T] int32: per-step argmax over classes, first index wins ties; 0 for a step whose log-probs are NaN (a NaN or +inf
 *              logit, or nothing but -inf), as ocrvi_ctc_greedy gives -- always inside [0, num_classes) (may be NULL)
 *   ids [B,T] int32: greedy CTC path after collapsing repeats and dropping `blank_id`, padded with -1
 *   lens [B] int32: number of valid entries of each ids row
 * ids/lens may both be NULL.  Mapping ids -> text (which also drops pad id 1, tokenizer.py:73) is host work. */
int ocrvi_rec_forward(ocrvi_rec* h, const float* x, int B, int H, int W,
                      float* log_probs, int32_t* argmax_ids, int32_t* ids, int32_t* lens,
                      void* workspace, size_t workspace_bytes, void* stream);
/* ocrvi_rec_forward with the confidence outputs of ocrvi_ctc_greedy_conf (defined there): best_lp [B,T] float32, char_lp [B,T] float32,
 * char_span [B,T,2] int32, computed from the log-probabilities this forward produces whether or not log_probs is stored.  Any output may be
 * NULL; log_probs, argmax_ids, ids and lens are bit-equal to what ocrvi_rec_forward writes for the same input.  Same workspace as
 * ocrvi_rec_forward (ocrvi_rec_workspace_bytes); enqueue-only, so it can be captured into a graph. */
int ocrvi_rec_forward_conf(ocrvi_rec* h, const float* x, int B, int H, int W,
                           float* log_probs, int32_t* argmax_ids, int32_t* ids, int32_t* lens,
                           float* best_lp, float* char_lp, int32_t* char_span,
                           void* workspace, size_t workspace_bytes, void* stream);
/* Test hook: float32 copies of backbone_norm output [B, H/16*W/4, D] (svtrv2.py:500) and FRM output
 * [B, W/4, D] (svtrv2.py:247).  Either may be NULL.  Must follow a forward on the same workspace/stream. */
int ocrvi_rec_status(const ocrvi_rec* h);   /* as ocrvi_det_status */
int ocrvi_rec_debug_features(ocrvi_rec* h, int B, int H, int W, float* backbone_norm, float* frm,
                             void* workspace, size_t workspace_bytes, void* stream);

/* The per-device f16x2 range flag behind ocrvi_{det,rec}_status: reset (asynchronous on `stream`) / read (synchronises the device). */
int ocrvi_range_reset(int device, void* stream);
int ocrvi_range_flag(int device, int* raised);

/* Standalone greedy CTC decode of caller-supplied log-probs: replaces SVTRv2.decode_probs' tensor half
 * (svtrv2.py:555-566).  log_probs [T,B,C] float32 on device. */
int ocrvi_ctc_greedy(int device, const float* log_probs, int T, int B, int C, int blank_id,
                     int32_t* argmax_ids, int32_t* ids, int32_t* lens, void* stream);

/* ocrvi_ctc_greedy with confidences: how sure the greedy path was of each character it kept, and which steps the character covers.
 * argmax_ids, ids and lens are exactly what ocrvi_ctc_greedy writes.  argmax_ids and best_lp are required, the rest may be NULL.
 *   best_lp [B,T] float32, laid out like argmax_ids: best_lp[b,t] is the float32 that log_probs[t,b,argmax_ids[b,t]] holds, bit for bit
 *     (for a step whose log-probs are NaN the argmax is 0 and best_lp is that NaN).
 *   Character k of row b, 0 <= k < lens[b], is emitted at step t0, the k-th step with am[t0] != blank_id && am[t0] != am[t0-1] (am =
 *     argmax_ids[b]; step 0 has no predecessor).  Its run is [t0, t1], t1 the last step such that am[t0..t1] are all equal.
 *   char_span [B,T,2] int32: (t0, t1) of character k; (-1, -1) for k >= lens[b].
 *   char_lp [B,T] float32: the maximum of best_lp[b, t0..t1] under fmaxf, so a NaN step is ignored unless every step of the run is NaN;
 *     -inf for k >= lens[b].
 * One wave per row, 64 steps per pass; a run that crosses a pass boundary is carried in registers and stored once, when it closes. */
int ocrvi_ctc_greedy_conf(int device, const float* log_probs, int T, int B, int C, int blank_id,
                          int32_t* argmax_ids, int32_t* ids, int32_t* lens, float* best_lp, float* char_lp, int32_t* char_span, void* stream);

/* ------------------------------------------------------------------------------------------------
 * CTC prefix beam search: the nbest most probable labellings of every row, each with its log-probability.  No counterpart in the
 * reference.  The standard prefix beam search without a language model, made deterministic by a tie rule and exact by string identity.
 * ------------------------------------------------------------------------------------------------
 * Row b of log_probs [T,B,C] float32 (device), blank = blank_id, beam width W = beam; all arithmetic in float64.
 *   Inputs.  v(t,c) = (double) log_probs[t,b,c].  A NaN is taken as -inf (probability 0).  +inf is not supported: the result is
 *     unspecified, and no address outside the buffers is formed.
 *   logsumexp.  lse(a,b) = m + log(exp(a-m) + exp(b-m)) with m = max(a,b); -inf when m is (the lse3 of ocrvi_ctc_loss with a third term
 *     of -inf).  a + b is -inf when either term is.
 *   Entry.  A beam entry is (prefix l, pb, pnb): pb the log-probability of all alignments of l so far that end in blank, pnb of those that
 *     end in a non-blank; s = lse(pb, pnb).  Start: one entry ((), 0, -inf).  Entries are kept in rank order i = 0..n-1.
 *   Step t, for entry i:
 *     stay (candidate index i*C + blank, prefix l_i): pb' = s_i + v(t,blank); pnb' = pnb_i + v(t,last(l_i)), -inf for the empty prefix.
 *     extend by c, c != blank (candidate index i*C + c, prefix l_i + c): pb' = -inf; pnb' = (c == last(l_i) ? pb_i : s_i) + v(t,c).
 *     merge: if l_i + c is, as a string of ids, the prefix l_j of another entry j of the beam, the extension is no candidate of its own:
 *       its pnb' is added with lse into the pnb' of j's stay candidate.  At most one i extends into a given j.  Identity is the id string
 *       itself (a hash filters, equality of the ids decides).
 *     Every class is extended: there is no top-k pruning of classes.
 *   Select.  A candidate's total is lse(pb', pnb').  Candidates with total -inf are dropped.  The W largest totals survive, larger first;
 *     equal totals are ordered by smaller candidate index.  That order is the next step's rank order.
 *   Output after step T-1, the first nbest entries in rank order: ids [B,nbest,T] int32 (the prefix, -1 beyond it), lens [B,nbest] int32,
 *     score [B,nbest] float64 = s.  A missing hypothesis (fewer than nbest finite ones) has lens = -1, score = -inf, ids = -1.  Pad id 1 is
 *     an ordinary label here, as it is for ocrvi_ctc_greedy.
 * score is a lower bound of the labelling's full probability: score[n] <= -ocrvi_ctc_loss(ids[n]), with equality when nothing that leads
 * to that labelling was ever pruned.  beam = 1 is not the greedy decode in general.
 * Limits: 1 <= nbest <= beam <= OCRVI_CTC_BEAM_MAX, 2 <= C <= 1024, 0 <= blank_id < C, 1 <= T <= OCRVI_CTC_BEAM_MAX_T, B >= 1; anything
 * else (or a null pointer, a workspace not 256-byte aligned) is OCRVI_EINVAL before any launch.  workspace: ocrvi_ctc_beam_workspace_bytes
 * (the prefixes of both beam tables, [B][2][beam][T rounded up to even] int16, rounded up to 256 bytes); OCRVI_ENOMEM when it is short.
 * Enqueue-only: one launch, no allocation, no synchronisation, capturable; the same input gives the same bytes.
 * One workgroup of 256 threads per row; the beam tables and two rows of v live in LDS, the prefixes too when both tables fit in 32 KiB
 * (in the workspace otherwise); selection is up to W rounds of a workgroup arg-max over candidates that are recomputed, never stored. */
#define OCRVI_CTC_BEAM_MAX 64
#define OCRVI_CTC_BEAM_MAX_T 1024
int ocrvi_ctc_beam_workspace_bytes(int T, int B, int C, int beam, size_t* bytes);
int ocrvi_ctc_beam(int device, const float* log_probs, int T, int B, int C, int blank_id, int beam, int nbest,
                   int32_t* ids, int32_t* lens, double* score, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Character n-gram language model: a backoff table over the recogniser's class ids, for ocrvi_ctc_beam_lm below.  No counterpart in the
 * reference.
 * ------------------------------------------------------------------------------------------------
 *   Symbols.  Class ids 0..C-1, C = num_classes, 2 <= C <= 1024.  The blank id never occurs in a labelling; in an n-gram it stands for
 *     begin of line (BOS = bos_id = the blank id) and is legal only as the FIRST symbol of a gram.  The 1-gram (BOS) is a context only: it
 *     carries a backoff weight and its lp is 0 (a non-zero lp there would predict the blank, which is refused).  There is no end-of-line
 *     term: a string's score does not depend on the line ending after it (out of scope).
 *   Order.  N = order, 1 <= N <= OCRVI_LM_MAX_ORDER.  The context of the prediction that follows the labelling l is
 *     ctx(l) = the last min(N-1, len(l)+1) symbols of BOS + l  (nothing for N = 1; (BOS) for the empty labelling when N >= 2).
 *   Key.  The n-gram g_1..g_k (g_1 the oldest symbol, 1 <= k <= N) is the 63-bit key (k << 60) | sum_j g_j << (10 (j-1)).  Never zero, never
 *     shared by two grams: the key is the gram, not a hash of it.
 *   Slot.  16 bytes {uint64 key; float lp; float bo}: lp = ln p(g_k | g_1..g_k-1), bo = the ln backoff weight of the gram as a context.
 *     Natural logarithms, finite float32, widened to float64 where they are used.
 *   Table.  Open addressing over cap = 1 << log2cap slots, cap >= 2 * entries (and >= 2); home slot (key * 0x9e3779b97f4a7c15 mod 2^64)
 *     >> (64 - log2cap); linear probing with wrap-around; key 0 = empty.  A gram is present iff a probe from its home meets its key before
 *     an empty slot.
 *   Blob.  A 48-byte header {uint32 magic 0x4d4c434f; uint32 version 1; int32 order, num_classes, bos_id, log2cap; uint64 entries;
 *     double unk_lp; uint64 reserved}, then the cap slots.  Little endian.  ocrvi_lm_build inserts the grams in the order given.
 *   Score.  lm(c | h) for a label c != blank and a context h of |h| symbols:  acc = 0;  for k = |h| down to 0:  if the gram h[-k:] + c
 *     (the last k symbols of h, then c) is present: return acc + lp of it;  else if k >= 1 and the gram h[-k:] is present: acc = acc + bo
 *     of it.  When the loop ends (the unigram of c is absent): return acc + unk_lp, unk_lp finite.  All sums float64, in this order.
 *   String.  g(()) = 0, g(l + c) = g(l) + lm(c | ctx(l)): float64 sums in prefix order, so g is a function of the id string alone, bit
 *     for bit.
 * Host entries (no device, no GPU needed):
 *   ocrvi_lm_build: n_grams grams, gram i = gram_ids[i][0 .. gram_lens[i]) of gram_ids [n_grams][OCRVI_LM_MAX_ORDER] int32 (the rest of a row
 *     is ignored) with lp[i], bo[i] -> the blob.  blob == NULL: *blob_bytes = its size (after every check).  OCRVI_EINVAL with a message for
 *     a gram given twice, a length outside 1..order, an id outside [0, num_classes), BOS anywhere but first, the blank as a predicted symbol
 *     (the 1-gram (BOS) with lp != 0), a non-finite lp / bo / unk_lp, order outside 1..6, num_classes outside 2..1024, bos_id outside
 *     [0, num_classes); OCRVI_ENOMEM when blob_capacity is short.
 *   ocrvi_lm_score: ids[0..len) labels (not the blank, < num_classes: OCRVI_EINVAL otherwise) -> *total = g(ids) and, if per_char is not
 *     NULL, per_char[q] = lm(ids[q] | ctx(ids[0..q))), float64.  Validates the blob as ocrvi_lm_create does.
 *   ocrvi_lm_create: validates the WHOLE blob on the host (header fields and magic, size == 48 + 16 * cap, entries == occupied slots <=
 *     cap / 2 -- so an empty slot exists and every probe ends --, every key's length tag in 1..order with no bit set beyond its symbols, ids
 *     < num_classes, BOS only first, finite lp / bo / unk_lp, every key where a probe from its home finds it) and uploads the slots to
 *     `device`: OCRVI_EINVAL with a message otherwise.  The kernel then never distrusts the table.  The handle owns the device copy, is
 *     read-only afterwards and may serve any number of concurrent searches on its device.  ocrvi_lm_destroy(NULL) is a no-op. */
#define OCRVI_LM_MAX_ORDER 6
typedef struct ocrvi_lm ocrvi_lm;
int ocrvi_lm_build(const int32_t* gram_ids, const int32_t* gram_lens, const float* lp, const float* bo, size_t n_grams, int order,
                   int num_classes, int bos_id, double unk_lp, void* blob, size_t blob_capacity, size_t* blob_bytes);
int ocrvi_lm_score(const void* blob, size_t blob_bytes, const int32_t* ids, int len, double* total, double* per_char);
int ocrvi_lm_create(int device, const void* blob, size_t blob_bytes, ocrvi_lm** out);
void ocrvi_lm_destroy(ocrvi_lm* h);

/* ------------------------------------------------------------------------------------------------
 * CTC prefix beam search with LM fusion (shallow fusion of the character n-gram model above; Hannun et al. 2014).  The definition is
 * ocrvi_ctc_beam's, word for word, with three additions:
 * ------------------------------------------------------------------------------------------------
 *   Rank total.  An entry also carries g_i = g(l_i) and len_i = len(l_i); the start entry has g = 0, len = 0.  The rank total of (s, g, len)
 *     is R = (s + alpha * g) + beta * len in float64: each product and each sum rounded on its own, no fused multiply-add.  alpha (LM
 *     weight) and beta (length bonus per character) are finite, alpha >= 0.
 *   Candidates.  The stay candidate of entry i keeps g_i and len_i; the extension by c has g_i + lm(c | ctx(l_i)) and len_i + 1.  pb', pnb',
 *     the repeat rule and the merge by id-string identity with lse are exactly ocrvi_ctc_beam's; a merged extension adds only its acoustic
 *     pnb' (the string is j's, so g and len already agree).  A candidate whose ACOUSTIC total lse(pb', pnb') is -inf is dropped.  Select
 *     takes the W largest R, equal R by the smaller candidate index i*C + c; that order is the next step's rank order.
 *   Outputs.  ids, lens as ocrvi_ctc_beam; score [B,nbest] float64 = R; ctc_score [B,nbest] float64 = s; lm_score [B,nbest] float64 = g.
 *     A missing hypothesis has lens = -1, ids = -1 and -inf in all three.
 * With alpha = beta = 0 and any valid model, ids, lens and score are ocrvi_ctc_beam's byte for byte, and ctc_score == score.
 * lm_score is g(ids) exactly (the same doubles added in the same order as ocrvi_lm_score adds them).
 * OCRVI_EINVAL before any launch, outputs untouched: every case of ocrvi_ctc_beam; a NULL handle or one ocrvi_lm_create did not return
 * (or of another device); handle num_classes != C; handle bos_id != blank_id; alpha or beta not finite, or alpha < 0; a score array not
 * 8-byte aligned.  workspace: ocrvi_ctc_beam_lm_workspace_bytes = ocrvi_ctc_beam's prefixes, then [B][beam][C] float64 (row `slot` of a
 * beam row holds lm(c | ctx(l)) for every c, for the one live prefix l that owns the slot), each part rounded up to 256 bytes;
 * OCRVI_ENOMEM when it is short.  Enqueue-only: one launch for all T steps, no allocation, no synchronisation, capturable; the same input
 * gives the same bytes.
 * One workgroup of 256 threads per row.  lm(c | ctx(l)) depends on the prefix alone: its C terms are looked up once, when an extension
 * creates the prefix (16-byte probes of the read-only table; the unigram level sits in LDS), and a staying entry keeps its slot, so a
 * candidate is two reads and two adds.  Selection: every class keeps the best candidate over the entries; a round is a workgroup arg-max
 * over the classes, after which one wave scans the winner's class again, lane i the entry i. */
int ocrvi_ctc_beam_lm_workspace_bytes(int T, int B, int C, int beam, size_t* bytes);
int ocrvi_ctc_beam_lm(int device, const float* log_probs, int T, int B, int C, int blank_id, int beam, int nbest, const ocrvi_lm* lm,
                      double alpha, double beta, int32_t* ids, int32_t* lens, double* score, double* ctc_score, double* lm_score,
                      void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Pre-processing on the device (the callers either side of the two models on the e2e path).
 * ------------------------------------------------------------------------------------------------ */
/* Replaces the detection input normalisation of src/pipeline/pipeline2.py:312-314: images uint8 HWC
 * [N,H,W,3] (device) -> float32 NCHW [N,3,H,W] = ((v/255 as float32) - mean) / std evaluated in float64. */
int ocrvi_normalize_u8(int device, const uint8_t* images, int N, int H, int W, float* out, void* stream);
/* Replaces the cv2.resize call of resize_image_for_det (src/pipeline/pipeline2.py:33-40): uint8 HWC [src_h,src_w,3] ->
 * uint8 HWC [dst_h,dst_w,3], OpenCV's 8-bit INTER_LINEAR (fixed-point) arithmetic. */
int ocrvi_resize_u8(int device, const uint8_t* src, int src_h, int src_w, uint8_t* dst, int dst_h, int dst_w, void* stream);
/* Replaces crop_image (src/det/test.py:123-130, box already reduced to its clamped bounding rect) followed by
 * preprocess_for_recognition (src/pipeline/pipeline2.py:92-128) for a batch of crops.  images uint8 HWC
 * [n_img,H,W,3]; boxes int32 [B,5] = (image index, x, y, w, h) in pixels, inside the image; out float32
 * [B,3,out_h,out_w].  w<=0 or h<=0 yields the all-zero tensor of pipeline2.py:154-156. */
int ocrvi_crop_resize_normalize(int device, const uint8_t* images, int n_img, int H, int W, const int32_t* boxes, int B,
                                int out_h, int out_w, float* out, void* stream);

/* Page table of the two *_pages entries below: int64 [n][OCRVI_PAGE_ENTRY] in DEVICE memory, entry i = (device address of page i, a
 * uint8 HWC [h,w,3] image, h, w, 0).  The kernels read it when they run, not when they are enqueued: a graph captured over these calls
 * stays valid when the pages are moved and only the table's contents are rewritten.  An entry with a null address or a side <= 0 is
 * invalid (it is never dereferenced). */
#define OCRVI_PAGE_ENTRY 4
/* Replaces the per-image resize_image_for_det (src/pipeline/pipeline2.py:33-40) + normalisation (:312-314) for n pages of their own
 * sizes that map to one H x W detector shape: out float32 NCHW [n,3,H,W] (16-byte aligned, W % 4 == 0), element for element equal to
 * ocrvi_resize_u8(page i -> H x W) followed by ocrvi_normalize_u8 on page i alone (an invalid entry gives the normalised zero pixel).
 * Enqueue-only on `stream`. */
int ocrvi_resize_normalize_pages(int device, const int64_t* pages, int n, int H, int W, float* out, void* stream);
/* ocrvi_crop_resize_normalize (crop_image, src/det/test.py:123-130 + preprocess_for_recognition, pipeline2.py:92-128) for crops of
 * pages of different sizes: boxes int32 [B,5] = (page table index, x, y, w, h); each output equals ocrvi_crop_resize_normalize on that
 * crop's page alone.  w<=0, h<=0, an index outside [0, n_pages) or an invalid entry yields the all-zero tensor (pipeline2.py:154-156).
 * Enqueue-only on `stream`. */
int ocrvi_crop_resize_normalize_pages(int device, const int64_t* pages, int n_pages, const int32_t* boxes, int B, int out_h, int out_w,
                                      float* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Four-point page rectification: the geometric half of the reference's stage 1, `--preprocess` (src/pipeline/pipeline2.py:291-302 ->
 * preprocess_image, src/preprocess/scanner.py:168-196 -> four_point_transform, scanner.py:29-53).  Finding the document's corners (scanner.py:78-132)
 * is "Document finder" below: the rembg network stays out, its contour half and a mask of the library's own are built; enhance_document (scanner.py:55-76) is below (the pipeline passes
 * enhance=False).
 * ------------------------------------------------------------------------------------------------ */
/* Host only, needs no GPU.  Replaces order_points (scanner.py:13-27), the output size (scanner.py:36-42), the destination corners
 * (scanner.py:44-48) and cv2.getPerspectiveTransform (scanner.py:50).  pts: four (x, y) corners of the document in the image, any order.
 *   order    x + y and y - x in float64; top-left = argmin of the sum, bottom-right = argmax, top-right = argmin of the difference,
 *            bottom-left = argmax; the first index wins ties (numpy).  The ordered corners are kept as float32.
 *   size     the four side lengths in float32 throughout (differences, squares, sum, correctly rounded sqrt), each truncated by int();
 *            *out_w = max(top, bottom), *out_h = max(left, right).
 *   corners  the destination corners (0,0), (w-1,0), (w-1,h-1), (0,h-1) as float32.
 *   m_fwd    [9] row-major, source -> destination (may be NULL): the 8 x 8 linear system of the four correspondences with h22 = 1, solved
 *            in double by Gaussian elimination with partial pivoting.
 *   m_inv    [9] destination -> source, what the warp entries below take: adjugate of m_fwd over its determinant, in double.
 * OCRVI_EINVAL with a message when out_w < 1 or out_h < 1, when the system is singular (three of the ordered corners on one line, or
 * two of them equal) or when the determinant is 0, and for non-finite corners.  The ordering can pick one point twice -- the diamond
 * (10,0) (20,10) (10,20) (0,10) orders to (10,0) (10,0) (20,10) (10,20) --; the reference then hands cv2 a degenerate system, this
 * entry refuses. */
int ocrvi_four_point_transform(const double* pts /*[4][2]*/, double* m_fwd /*[9]*/, double* m_inv /*[9]*/, int32_t* out_w, int32_t* out_h);
/* Replaces cv2.warpPerspective(image, M, (w, h)) as four_point_transform calls it (scanner.py:51: bilinear, constant border 0):
 * src uint8 HWC [src_h,src_w,3] -> dst uint8 HWC [dst_h,dst_w,3], both DEVICE; m_inv_host: HOST [9] destination -> source (it is copied
 * into the launch: free again on return).  Enqueue-only on `stream`, graph-capturable: no allocation, no synchronisation.
 * The arithmetic is the library's own definition, modelled on OpenCV's classic fixed-point bilinear remap.  OpenCV's own implementation
 * differs between versions and between its block sizes and cv2 is absent from the build container: parity with cv2 is UNPINNED, as for
 * ocrvi_resize_u8.  For destination pixel (x, y) and m = m_inv:
 *   X0 = (m0 x + m1 y) + m2,  Y0 = (m3 x + m4 y) + m5,  W0 = (m6 x + m7 y) + m8   IEEE double, in this order, no fused multiply-add
 *   s  = W0 != 0 ? 32.0 / W0 : 0.0
 *   X  = rint(clamp(X0 s, -2147483648.0, 2147483647.0)) as int32, round half to even (a NaN product counts as the lower bound); Y likewise
 *   sx = X >> 5 (arithmetic), ax = X & 31; sy, ay likewise
 *   weights (32-ax)(32-ay) 32, ax (32-ay) 32, (32-ax) ay 32, ax ay 32 (sum 32768) on the taps (sy, sx), (sy, sx+1), (sy+1, sx), (sy+1, sx+1);
 *   a tap outside [0,src_h) x [0,src_w) contributes 0 (decided on the integers: no address is formed for it)
 *   out_c = (sum w p_c + 16384) >> 15
 * No alignment is asked of src or dst (a dst that is a multiple of 4 is written in 4-byte words). */
int ocrvi_warp_perspective_u8(int device, const uint8_t* src, int src_h, int src_w, const double* m_inv_host /*[9]*/,
                              uint8_t* dst, int dst_h, int dst_w, void* stream);
/* The same warp for n pages in one launch (1 <= n <= 65535): src_pages and dst_pages are page tables as above (OCRVI_PAGE_ENTRY), m_inv
 * DEVICE float64 [n][9]; page i of dst_pages = ocrvi_warp_perspective_u8 of page i of src_pages under matrix i, bit for bit.  Tables,
 * matrices and pages are read when the kernel runs: a captured graph survives moved pages and rewritten tables and matrices.  A
 * destination whose source entry is invalid is filled with 0; an invalid destination entry is skipped and never dereferenced.
 * Destination addresses need no alignment.  Enqueue-only on `stream`. */
int ocrvi_warp_perspective_pages(int device, const int64_t* src_pages, const int64_t* dst_pages, const double* m_inv /*DEVICE [n][9]*/, int n,
                                 void* stream);

/* ------------------------------------------------------------------------------------------------
 * Oriented text crops (opt-in; the default stays the reference's rectangle crop, crop_image, src/det/test.py:123-130): the minimum-area
 * rectangle of each DB polygon, warped and resized into the recogniser's batch in one launch.  The reference carries only the left-overs
 * of this path (DBPostProcessor.min_size, is_output_polygon, src/det/test.py:52,55).  The definitions below are the library's own and
 * exact; parity with cv2.minAreaRect / PaddleOCR unpinned (cv2 absent).  tests/quad_ref.py restates them in Python integers.
 * ------------------------------------------------------------------------------------------------ */
/* Host only, needs no GPU.  points int32 [total][2]; offs int32 [n+1]: polygon i = points[offs[i] .. offs[i+1]); quads float64 [n][4][2];
 * flags int32 [n].  Coordinates lie in [-32768, 32767], anything else is OCRVI_EINVAL.
 *   hull       the distinct points sorted by (x, y); the strictly convex hull by the monotone chain, lower chain then upper chain: a point is
 *              kept only while every integer cross product is > 0, so collinear points are dropped; hull[0] is the smallest (x, y).
 *              Fewer than three hull vertices: flags[i] = 1 (degenerate) and the quad is the four corners (x0,y0) (x1,y0) (x1,y1) (x0,y1) of
 *              the polygon's inclusive bounding box (all zero for a polygon without points).  Otherwise flags[i] = 0.
 *   rectangle  for hull edge k = hull[k] -> hull[k+1]: d = (dx, dy), n = (-dy, dx); s_min, s_max = the extremes of p.d and t_min, t_max of
 *              p.n over the hull vertices (int64); area = (s_max - s_min)(t_max - t_min) / |d|^2, compared as exact rationals (128-bit cross
 *              multiplication).  The smallest area wins, the smallest k on a tie.
 *   corners    in the order (s_min, t_min), (s_max, t_min), (s_max, t_max), (s_min, t_max): x = (s dx - t dy) / |d|^2, y = (s dy + t dx) /
 *              |d|^2; each numerator is an exact integer below 2^53, converted to double and divided once. */
int ocrvi_min_area_quads(const int32_t* points, const int32_t* offs, int n, double* quads /*[n][4][2]*/, int32_t* flags /*[n]*/);
/* Host only.  The crop descriptors of n quads: crops int32 [n][4] = (page_ids[i], w, h, 0), m_inv float64 [n][9] destination -> source;
 * page_ids int32 [n] (the page table index of each quad's page), page_hw int32 [n][2] = that page's (height, width).
 * Quad i goes through the geometry of ocrvi_four_point_transform (corner order, float32 side lengths truncated to w and h, the 8 x 8
 * solve); w, h and its m_inv are stored.  When that geometry refuses the quad (w < 1 or h < 1, a singular system, the ordering picking one
 * corner twice -- a rectangle tilted by exactly 45 degrees --) or flags[i] != 0, the descriptor falls back to the reference's crop: with
 * x0 = floor(min x), y0 = floor(min y), bw = ceil(max x) - x0 + 1, bh = ceil(max y) - y0 + 1 over the four corners (for a flagged quad:
 * cv2.boundingRect of the polygon), x = max(0, x0), y = max(0, y0), w = min(bw, page_w - x), h = min(bh, page_h - y) (src/det/test.py:
 * 126-129) and m_inv = [1,0,x, 0,1,y, 0,0,1]; a rectangle that is empty after clamping gets w = h = 0.  Under the warp below an integer
 * translation reads the page's pixels unchanged, so a fallback crop is that rectangle of the page bit for bit.  For a flagged polygon the
 * rectangle is the reference's (crop_rect of the polygon).  For a refused quad it is the bounding box of the quad's corners, which contains
 * the polygon's bounding rectangle and can be larger than it (the entry sees the quad, not the polygon): no parity with the rectangle
 * mode is claimed there.  A refused quad leaves ocrvi_last_error empty.  Corners must be finite and within +-2^20 (OCRVI_EINVAL).  No 90-degree turn: a quad that comes out taller than wide stays so. */
int ocrvi_quad_crops(const double* quads, const int32_t* flags, int n, const int32_t* page_ids, const int32_t* page_hw /*[n][2]*/,
                     int32_t* crops /*[n][4]*/, double* m_inv /*[n][9]*/);
/* The oriented analogue of ocrvi_crop_resize_normalize_pages.  pages: a page table (OCRVI_PAGE_ENTRY); crops int32 [B][4] and m_inv float64
 * [B][9] as above, both in DEVICE memory; out float32 [B,3,out_h,out_w].  Enqueue-only on `stream`: no allocation, no synchronisation;
 * tables, descriptors and pages are read when the kernel runs, so a captured graph survives rewritten descriptors.
 * Output b is the composition of two definitions above.  First the intermediate crop C_b, uint8 [h, w, 3]: the warp of
 * ocrvi_warp_perspective_u8 under m_inv[b] -- the same 1/32-pixel coordinates, IEEE double arithmetic in the stated order without fused
 * multiply-add, 15-bit weights and (sum + 16384) >> 15 -- with one difference: a tap's row and column are clamped to the page (replicate
 * border) instead of contributing 0, so a crop that overhangs the page edge gains no black rim.  Then the rest of
 * ocrvi_crop_resize_normalize applied to the whole of C_b: new_w = int(w * (out_h / h)) squashed to out_w and at least 1, the exact-2x box
 * filter, the fixed-point bilinear resize, right padding with 255, the float32 normalisation.  C_b is never written to memory.  When out_w
 * is a multiple of 4, out is 16-byte aligned, B <= 65535 and out_h <= 62, a workgroup per out_h x 64 tile warps the pixels of C_b the tile
 * reads once into LDS and resizes from there (16-byte stores); otherwise a thread per output pixel forms the at most 2 x 2 pixels of C_b it
 * reads.  Both forms write the same bits.  w <= 0, h <= 0, an index outside [0, n_pages) or an invalid table entry yields the all-zero
 * tensor. */
int ocrvi_crop_quad_resize_normalize_pages(int device, const int64_t* pages, int n_pages, const int32_t* crops, const double* m_inv, int B,
                                           int out_h, int out_w, float* out, void* stream);
/* The same for crops of one uint8 [n_img,H,W,3] array (the analogue of ocrvi_crop_resize_normalize): crops[b][0] is the image index. */
int ocrvi_crop_quad_resize_normalize(int device, const uint8_t* images, int n_img, int H, int W, const int32_t* crops, const double* m_inv,
                                     int B, int out_h, int out_w, float* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * enhance_document, the reference's "Magic Color" (src/preprocess/scanner.py:55-76): COLOR_BGR2LAB (:60), CLAHE(clipLimit 2.0, 8 x 8 tiles)
 * on L (:63-64), COLOR_LAB2BGR (:67), fastNlMeansDenoisingColored(h 10, hColor 10, template 7, search 21) (:70), filter2D with the 3 x 3
 * sharpen kernel (:73-74).  The reference's constants are fixed: none is a parameter.
 * Pages are RGB uint8 HWC [h,w,3] in DEVICE memory, 16 <= h, w and h w <= 2^29 (the 13-pixel reflection and the 8 x 8 grid need 16); Lab
 * pages have the same layout with (L, a, b) in the three bytes.  The Lab of an RGB pixel is the reference's COLOR_BGR2LAB of the swapped
 * pixel and the other stages treat the channels alike, so no channel swap is needed anywhere.
 * The arithmetic is the library's own definition, modelled on OpenCV's 8-bit integer paths and stated in full here.  OpenCV's Lab, CLAHE
 * and NLM code differ between versions and cv2 is absent from the build container: parity with cv2 is UNPINNED, as for ocrvi_resize_u8 and
 * the warp.  Everything on the device is integer: tests/enhance_ref.py restates it in numpy and the kernels are bit-equal to it.
 *
 * Tables: built on the host in double, each entry rounded with rint, uploaded once per device by ocrvi_enhance_init.  g is the sRGB
 * decode (c <= 0.04045 ? c / 12.92 : ((c + 0.055) / 1.055)^2.4), g^-1 the sRGB encode (l <= 0.0031308 ? 12.92 l : 1.055 l^(1/2.4) - 0.055),
 * f(t) = cbrt(t) for t > 216/24389, else (841/108) t + 4/29.  M is OpenCV's sRGB -> XYZ D65 matrix (0.412453 0.357580 0.180423 / 0.212671
 * 0.715160 0.072169 / 0.019334 0.119193 0.950227), white its row sums.
 *   LIN[256]  = rint(2040 g(v / 255))                  F[2041]  = rint(32768 f(t / 2040))          ENC[2041] = rint(255 g^-1(t / 2040))
 *   FY[256]   = rint((L 100 / 255 + 16) / 116 * 32768) DA[256]  = rint((a - 128) 32768 / 500)      DB[256]   = rint((b - 128) 32768 / 200)
 *   W1[1024], W2[1024]: WC[k] = rint(255 exp(-(k 64 / 49) / (100 C))) for C = 1, 2 (last non-zero entry: k = 477, k = 954)
 *   CF[3][3]  = rint(4096 M[i][j] / white[i])          CI[3][3] = rint(4096 M^-1[i][j] white[j])   (M^-1 = adjugate / determinant); in each
 *               row the entry of largest magnitude is then adjusted so that the row sums to exactly 4096
 * RGB -> Lab:  l = LIN[rgb];  XYZ = (CF l + 2048) >> 12 (each <= 2040);  fX, fY, fZ = F[XYZ];
 *   L = clamp((2958 fY - 13369344 + 163840) // 327680, 0, 255);  a = clamp(((500 (fX - fY) + 16384) >> 15) + 128, 0, 255);
 *   b = clamp(((200 (fY - fZ) + 16384) >> 15) + 128, 0, 255).  Shifts are arithmetic, // is floor division.
 * Lab -> RGB:  fy = FY[L], fx = fy + DA[a], fz = fy - DB[b], each clamped to [0, 49151];
 *   t(f) = (f^3 2040 + 2^44) >> 45 in 64 bits for f > 6781, else max(((f - 4520) 8383 + 2^19) >> 20, 0);
 *   r = clamp((CI t + 2048) >> 12, 0, 2040);  out = ENC[r].
 * CLAHE on channel 0 (a and b are copied):  Hp, Wp = h, w rounded up to multiples of 8, the plane extended right and down by reflect-101;
 *   th = Hp / 8, tw = Wp / 8.  Per tile, on its 256-bin histogram: clip = max(2 th tw // 256, 1); excess = sum max(hist - clip, 0);
 *   hist = min(hist, clip) + excess // 256; r = excess % 256; if r > 0, step = max(256 // r, 1) and bins 0, step, 2 step, ... get +1 each
 *   until r are given.  LUT[v] = (255 cdf(v) + th tw // 2) // (th tw).  For pixel (y, x) with level v: nx = 2x + 1 - tw, tx1 = floor(nx /
 *   2tw), ax = nx - tx1 2tw, tx2 = tx1 + 1, both clamped to [0, 7]; likewise in y; out = (sum of the four LUT[v] weighted by (2tw - ax | ax)
 *   (2th - ay | ay), + 2 tw th) // (4 tw th), in 64 bits.
 * NLM: once on the L plane with W1 and once on the (a, b) pair jointly with W2.  The page is extended by 13 pixels each side with
 *   reflect-101.  For pixel p and each of the 21 x 21 offsets q: D = sum over the 7 x 7 template t and the channels of the group of
 *   (I(p + t) - I(p + q + t))^2;  w = WC[min(D >> 6, 1023)];  out_c(p) = (sum_q w I_c(p + q) + floor(sum_q w / 2)) // sum_q w  (sum w >=
 *   255: q = 0 has D = 0; every sum fits int32).
 * Sharpen: per channel clamp(9 c - the eight neighbours, 0, 255), reflect-101 borders.
 * ------------------------------------------------------------------------------------------------ */
/* Builds the tables and uploads them to `device`; idempotent.  The only entry of this section that allocates or synchronises. */
int ocrvi_enhance_init(int device);
/* Host only, needs no GPU: the tables as int32, in the order LIN, F, ENC, FY, DA, DB, W1, W2, CF, CI (7172 values, 28688 bytes) -> out.
 * *bytes = the size; out == NULL asks for the size alone; OCRVI_ENOMEM when cap is smaller. */
int ocrvi_enhance_tables(void* out, size_t cap, size_t* bytes);
/* Scratch DEVICE memory of ocrvi_enhance_u8 for an h x w page: 16384 + 2 * (3 h w rounded up to a multiple of 256) bytes (the 64 tile
 * LUTs and two Lab / RGB pages). */
int ocrvi_enhance_workspace_bytes(int h, int w, size_t* bytes);
/* Replaces enhance_document(image) (scanner.py:55-76): the stages below in the reference's order -- rgb_to_lab, clahe_lab, lab_to_rgb,
 * rgb_to_lab, nlm_lab, lab_to_rgb, sharpen --, every stage boundary a uint8 page as there (two boundaries stay in registers: the bytes are
 * those of the composition).  No alignment is asked of src, dst or workspace (a multiple of 4 is read and written in 4-byte words).
 * All entries from here on are enqueue-only on `stream` and graph-capturable: no allocation, no synchronisation.  They return
 * OCRVI_EINVAL, with a message and without touching dst, for a null pointer, a side below 16, a dst that overlaps src and a device on
 * which ocrvi_enhance_init has not run; OCRVI_ENOMEM for a short workspace. */
int ocrvi_enhance_u8(int device, const uint8_t* src, int h, int w, uint8_t* dst, void* workspace, size_t workspace_bytes, void* stream);
/* The stages on their own (the same kernels).  cv2.cvtColor(COLOR_BGR2LAB) (scanner.py:60) / cv2.cvtColor(COLOR_LAB2BGR) (:67): */
int ocrvi_rgb_to_lab_u8(int device, const uint8_t* src, int h, int w, uint8_t* dst, void* stream);
int ocrvi_lab_to_rgb_u8(int device, const uint8_t* src, int h, int w, uint8_t* dst, void* stream);
/* cv2.createCLAHE(2.0, (8, 8)).apply on channel 0 of a Lab page (scanner.py:61-66); workspace: OCRVI_CLAHE_WORKSPACE_BYTES of DEVICE memory. */
#define OCRVI_CLAHE_WORKSPACE_BYTES 16384
int ocrvi_clahe_lab_u8(int device, const uint8_t* src, int h, int w, uint8_t* dst, void* workspace, size_t workspace_bytes, void* stream);
/* The Lab-space middle of cv2.fastNlMeansDenoisingColored(img, None, 10, 10, 7, 21) (scanner.py:70): Lab page -> Lab page. */
int ocrvi_nlm_lab_u8(int device, const uint8_t* src, int h, int w, uint8_t* dst, void* stream);
/* cv2.filter2D(img, -1, [[-1,-1,-1],[-1,9,-1],[-1,-1,-1]]) (scanner.py:73-74) on any 3-channel page. */
int ocrvi_sharpen_u8(int device, const uint8_t* src, int h, int w, uint8_t* dst, void* stream);

/* ------------------------------------------------------------------------------------------------
 * JPEG decode: replaces the cv2.imread at the head of the reference's loop (src/pipeline/pipeline2.py:284-288; its data are JPEG files,
 * src/det/dataloader.py:307).  The host half is one serial pass per file (markers, EXIF orientation, Huffman decoding); dequantisation,
 * inverse DCT, chroma upsampling, colour conversion and the orientation run on the device, batched over pages.
 * Supported: SOF0 / SOF1 (Huffman, 8-bit precision), one interleaved scan; 1 component (grey, written to all three channels as
 * IMREAD_COLOR does) or 3 (YCbCr) with chroma sampling 1 x 1 and luma sampling 1 x 1, 2 x 1 or 2 x 2 (4:4:4, 4:2:2, 4:2:0); 8- or 16-bit
 * quantisation tables; restart intervals; APPn / COM skipped except APP1-EXIF, of which tag 0x0112 of IFD0 is read (both byte orders).
 * Refused with OCRVI_EINVAL and a message naming the feature, never guessed and never decoded on the host instead: progressive,
 * arithmetic, lossless, hierarchical and 12-bit files, 4 components, an Adobe marker with transform 0 or component ids R, G, B without
 * JFIF (RGB-coded files), other sampling factors, several scans.  The bytes are untrusted: a truncated or corrupt file (bad marker
 * length, a code that is not in its table, a run past coefficient 63, a missing or misnumbered RSTn, data left over at an RSTn or after
 * the last MCU, no EOI, a side of 0 or above 65500, a missing table, a DC value outside 16 bits, fewer than two bits of scan data per
 * block) is OCRVI_EINVAL.
 * The arithmetic is the library's own definition, stated here; tests/jpeg_ref.py restates it in NumPy.  For files a conforming encoder
 * produced from 8-bit images it equals libjpeg-turbo's default decode (PIL's Image.open().convert("RGB")) bit for bit -- pinned by
 * tests/golden/jpeg_cases.npz; parity with cv2.imread is UNPINNED (cv2 absent).  For coefficients no encoder produces the two saturating
 * steps below are the definition (libjpeg-turbo's SIMD code saturates differently): there the claim is device == tests/jpeg_ref.py.
 *   dequantise  c = coefficient (int16) * table entry (<= 65535) in 32 bits, saturated to [-16384, 16383]
 *   IDCT        the 8 x 8 "slow integer" inverse DCT, 13-bit constants 2446 3196 4433 6270 7373 9633 12299 15137 16069 16819 20995 25172,
 *               the LL&M factorisation: even part from inputs 0, 2, 4, 6 (z1 = (i2 + i6) 4433, t2 = z1 - i6 15137, t3 = z1 + i2 6270,
 *               t0 = (i0 + i4) << 13, t1 = (i0 - i4) << 13), odd part from 1, 3, 5, 7.  Pass 1 down the columns, (x + 2^10) >> 11,
 *               saturated to [-16384, 16383]; pass 2 along the rows, (x + 2^17) >> 18, + 128, clamped to [0, 255].  Shifts are
 *               arithmetic.  With both saturations every true value is below 2^31, so 32-bit wrap-around arithmetic is exact.
 *   planes      component c is ceil(W h_c / hmax) x ceil(H v_c / vmax) samples; the block padding beyond them is never read
 *   4:2:2 rows  out[2i] = (3 c[i] + c[i-1] + 1) >> 2, out[2i+1] = (3 c[i] + c[i+1] + 2) >> 2, the first output c[0], the last c[last]
 *   4:2:0       t = 3 near_row + far_row (the row above the first / below the last real row is that row itself); out[2i] = (3 t[i] +
 *               t[i-1] + 8) >> 4, out[2i+1] = (3 t[i] + t[i+1] + 7) >> 4, (4 t[0] + 8) >> 4 and (4 t[last] + 7) >> 4 at the ends
 *   narrow      a chroma plane of one or two columns is replicated (each sample twice, in 4:2:0 in both directions) instead of filtered
 *   colour      cb = Cb - 128, cr = Cr - 128: R = Y + ((91881 cr + 32768) >> 16), G = Y + ((-22554 cb - 46802 cr + 32768) >> 16),
 *               B = Y + ((116130 cb + 32768) >> 16), each clamped to [0, 255]
 *   orientation EXIF value k as PIL.ImageOps.exif_transpose applies it (2 mirror, 3 rotate 180, 4 flip, 5 transpose, 6 rotate 90
 *               clockwise, 7 transverse, 8 rotate 90 counter-clockwise); 5..8 swap height and width
 * Coefficient stream (what ocrvi_jpeg_parse writes, little-endian 32-bit words): [blocks + 1] record offsets, then the records.  Block
 * d, in the order the scan codes the blocks (MCU by MCU; inside an MCU the luma blocks row by row, then Cb, then Cr; a grey file block
 * by block in raster order), owns records off[d] .. off[d+1]; off[0] = 0 and off[blocks] = the number of records.  A record is
 * (position << 16) | (value & 0xffff): position = row * 8 + column of a NON-ZERO quantised coefficient (the DC value after prediction),
 * value its int16; within a block DC first, then zigzag order.  Zero coefficients have no record: a page costs its entropy, not 3 H W.
 * ------------------------------------------------------------------------------------------------ */
typedef struct {
    int32_t width, height, components;      /* of the coded frame (before orientation) */
    int32_t h_samp[3], v_samp[3];           /* sampling factors per component (1 x 1 for a grey file; 0 for absent components) */
    int32_t restart_interval;               /* MCUs, 0 = none */
    int32_t orientation;                    /* EXIF 0x0112, 1..8; 1 when absent or malformed */
    int32_t out_height, out_width;          /* of the decoded page, after orientation */
    int32_t reserved;
    int64_t blocks;                         /* 8 x 8 blocks of the scan */
    uint64_t stream_bytes;                  /* a `cap` that ocrvi_jpeg_parse never exceeds: 4 (blocks + 1 + min(64 blocks, 4 x scan bytes + blocks)) */
    uint64_t workspace_bytes;               /* device bytes of the page's component planes, padded to whole MCUs, a multiple of 256 */
    uint16_t quant[3][64];                  /* the quantisation table of each component, natural (row-major) order */
    char reason[160];                       /* the message when the call fails (also ocrvi_last_error) */
} ocrvi_jpeg_info_t;
/* Host only, needs no GPU.  Parses the markers up to the scan.  On OCRVI_EINVAL the geometry fields are filled when the frame header was
 * reached.  Takes no lock and no interpreter state, like ocrvi_jpeg_parse: calls from a thread pool run in parallel. */
int ocrvi_jpeg_info(const void* data, size_t n, ocrvi_jpeg_info_t* info);
/* Host only.  Huffman-decodes the scan into the coefficient stream at out[0 .. cap) (4-byte aligned; pinned memory when it is to be
 * uploaded); *used = its bytes.  OCRVI_ENOMEM when cap is too small (never with cap >= info.stream_bytes). */
int ocrvi_jpeg_parse(const void* data, size_t n, void* out, size_t cap, size_t* used);
/* Host only.  Fills one entry of the table ocrvi_jpeg_decode_pages reads, int64 [OCRVI_JPEG_ENTRY]: (0 stream offset, 1 blocks, 2 records,
 * 3 width, 4 height, 5 components, 6 luma h, 7 luma v, 8 orientation, 9 destination offset, 10 destination row stride, 11 workspace
 * offset, 12..15 zero, 16..63 the three quantisation tables as uint16 [3][64]).  Offsets are in bytes from records_dev (a multiple of
 * 4), dst_base (signed: pages of one launch may lie in different buffers either side of dst_base) and workspace (a multiple of 8);
 * dst_stride >= 3 out_width. */
#define OCRVI_JPEG_ENTRY 64
int ocrvi_jpeg_table_entry(const ocrvi_jpeg_info_t* info, size_t used, int64_t stream_offset, int64_t dst_offset, int64_t dst_stride,
                           int64_t workspace_offset, int64_t* entry);
/* Decodes n_pages pages in two launches (jpeg_idct_kernel: records -> planes in the workspace; jpeg_rgb_kernel: planes -> uint8 HWC RGB
 * [out_height, out_width, 3] at dst_base + destination offset, rows dst_stride bytes apart; bytes between rows are not written).
 * records_dev: the pages' streams, table_dev: int64 [n_pages][OCRVI_JPEG_ENTRY], both DEVICE memory and read when the kernels run, so a
 * captured graph survives rewritten tables and streams.  Enqueue-only on `stream`: no allocation, no synchronisation.  The pages'
 * workspace regions must not overlap; an entry whose fields are out of range, or whose planes do not fit workspace_bytes, is skipped and
 * never dereferenced.  A destination that is 4-byte aligned with a 4-byte aligned stride is written in words. */
int ocrvi_jpeg_decode_pages(int device, const void* records_dev, const int64_t* table_dev, int n_pages, void* dst_base, void* workspace,
                            size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * PNG decode: the other format the reference's loop reads with cv2.imread (src/pipeline/pipeline2.py:264-268, :284-288; its dataloaders
 * take .png too, src/det/dataloader.py:307-311, src/rec2/dataloader.py:188).  The host half is what is serial per file: the chunk list,
 * CRC-32, inflate (written here: no zlib, no libpng) and Adler-32.  The host uploads what the file holds, not pixels; undoing the row
 * filters, unpacking bits, the palette lookup, dropping alpha and 16 -> 8 bit run on the device, batched over pages.
 * Accepted: all 15 legal pairs of colour type and bit depth (grey 1 2 4 8 16, RGB 8 16, palette 1 2 4 8, grey + alpha 8 16, RGBA 8 16);
 * any number of IDAT chunks, empty ones included; stored, fixed and dynamic deflate blocks; ancillary chunks (tRNS gAMA cHRM sRGB iCCP
 * bKGD pHYs eXIf tEXt ..., and APNG's acTL fcTL fdAT: the default image is decoded) are skipped by length, their CRC unread; bytes in
 * the IDAT data after the end of the zlib stream are ignored.
 * Refused with OCRVI_EINVAL and a message naming the feature, never guessed and never decoded by other means: Adam7 interlace, a
 * compression or filter method other than 0, an illegal type / depth pair, a side of 0 or above 65500, a colour-type-3 file without PLTE
 * before IDAT, a PLTE length that is no multiple of 3 or above 256 entries, an unknown critical chunk (Apple's CgBI among them), IDAT
 * chunks that are not consecutive.  The bytes are untrusted; each of these is OCRVI_EINVAL too: a truncated file, a wrong CRC on IHDR,
 * PLTE, IDAT or IEND (IDAT's is checked by ocrvi_png_parse, the others by ocrvi_png_info as well), a bad zlib header (CM != 8, a window
 * above 32 K, FCHECK, a preset dictionary), a reserved block type, a stored-block length whose complement does not match, an
 * over-subscribed code-length set, an incomplete one other than the single one-bit code zlib accepts (or no distance code at all), a code
 * with no symbol, a distance reaching before the start of the output, a wrong Adler-32, a missing IEND, output shorter or longer than
 * stream_bytes, a filter byte above 4.
 * Stream (what ocrvi_png_parse writes): for colour type 3 first a 1024-byte palette, 256 x (R, G, B, 0), zero beyond the file's PLTE
 * entries; then, for every colour type, the inflated scanlines exactly as the file holds them, height x (1 + row_bytes) bytes, each row
 * led by its filter byte; row_bytes = ceil(width x channels x bit_depth / 8).
 * The arithmetic is the library's own definition, stated here; tests/png_ref.py restates it in NumPy.  It equals PIL's
 * Image.open().convert("RGB") bit for bit for 14 of the 15 pairs (pinned by tests/golden/png_cases.npz); 16-bit grey (PIL maps it
 * differently) and palette indices beyond PLTE are pinned to tests/png_ref.py only; parity with cv2.imread is UNPINNED (cv2 absent).
 *   unfilter    bpp = max(1, channels x bit_depth / 8); a = the reconstructed byte bpp to the left, b = the byte above, c = the byte
 *               above-left (each 0 outside the row or the image); every reconstructed byte is (x + p) & 255 with p = 0, a, b,
 *               (a + b) >> 1 or Paeth for filter bytes 0 .. 4
 *   Paeth       q = a + b - c; a if |q - a| <= |q - b| and |q - a| <= |q - c|; else b if |q - b| <= |q - c|; else c
 *   samples     packed most significant bit first; grey samples of depth 1, 2, 4 scale by 255, 85, 17; a 16-bit sample gives its high
 *               byte; grey goes to all three channels; palette index i gives palette row i, rows beyond the file's PLTE are (0, 0, 0)
 *   ignored     alpha is dropped, never composited; tRNS, gamma, colour profiles and the eXIf orientation are not applied
 * ------------------------------------------------------------------------------------------------ */
typedef struct {
    int32_t width, height, bit_depth, colour_type;
    int32_t channels;                       /* samples per pixel: 1 (grey, palette), 2 (grey + alpha), 3 (RGB), 4 (RGBA) */
    int32_t row_bytes;                      /* ceil(width x channels x bit_depth / 8), without the filter byte */
    int32_t out_height, out_width;          /* of the decoded page (= height, width: no orientation is applied) */
    int32_t palette_entries;                /* of the file's PLTE, colour type 3 only; 0 otherwise */
    int32_t reserved;
    uint64_t idat_bytes;                    /* compressed bytes, all IDAT chunks together */
    uint64_t stream_bytes;                  /* the exact size of the page's stream */
    uint64_t workspace_bytes;               /* device bytes of the page's line between bands: 0 for a page of one band, a multiple of 256 */
    char reason[160];                       /* the message when the call fails (also ocrvi_last_error) */
} ocrvi_png_info_t;
/* Host only, needs no GPU.  Checks the signature, parses IHDR and walks the chunk list up to IEND.  On OCRVI_EINVAL the geometry fields
 * are filled when IHDR was reached.  Takes no lock and no interpreter state, like ocrvi_png_parse: calls from a thread pool run in
 * parallel. */
int ocrvi_png_info(const void* data, size_t n, ocrvi_png_info_t* info);
/* Host only.  Joins the IDAT chunks and inflates them into the page's stream at out[0 .. cap) (pinned memory when it is to be uploaded);
 * *used = info.stream_bytes.  Never writes past cap: OCRVI_ENOMEM when cap < info.stream_bytes. */
int ocrvi_png_parse(const void* data, size_t n, void* out, size_t cap, size_t* used);
/* Host only.  Fills one entry of the table ocrvi_png_decode_pages reads, int64 [OCRVI_PNG_ENTRY]: (0 stream offset, 1 stream bytes,
 * 2 width, 3 height, 4 bit depth, 5 colour type, 6 palette entries, 7 destination offset, 8 destination row stride, 9 workspace offset,
 * 10..15 zero).  Offsets are in bytes from streams_dev (a multiple of 4), dst_base (signed: pages of one launch may lie in different
 * buffers either side of dst_base) and workspace (a multiple of 4); dst_stride >= 3 out_width. */
#define OCRVI_PNG_ENTRY 16
int ocrvi_png_table_entry(const ocrvi_png_info_t* info, size_t used, int64_t stream_offset, int64_t dst_offset, int64_t dst_stride,
                          int64_t workspace_offset, int64_t* entry);
/* Host only.  What the kernel will do for the page: it walks the page in *bands bands of *band_rows rows (thread = row); inside a band
 * the rows run skewed by one step, a step reconstructing one chunk of *chunk_bytes bytes per row, so a band of r rows and c chunks per
 * row takes c + r - 1 steps; *steps = their sum over the bands.  Any of the four pointers may be null. */
int ocrvi_png_plan(const ocrvi_png_info_t* info, int* band_rows, int* chunk_bytes, int* bands, int* steps);
/* Decodes n_pages pages in one launch (png_unfilter_kernel, one workgroup per page) into uint8 HWC RGB [height, width, 3] at dst_base +
 * destination offset, rows dst_stride bytes apart; bytes between rows are not written.  streams_dev: the pages' streams, table_dev: int64
 * [n_pages][OCRVI_PNG_ENTRY], both DEVICE memory and read when the kernel runs, so a captured graph survives rewritten tables and
 * streams; the streams are not modified.  Enqueue-only on `stream`: no allocation, no synchronisation.  The pages' workspace regions must
 * not overlap (workspace may be null when workspace_bytes is 0: no page of more than one band).  An entry whose fields are out of range
 * or inconsistent -- stream bytes other than what width, height, depth and type imply, an illegal type / depth pair, a side of 0 or above
 * 65500, a stride below 3 width, a line that does not fit workspace_bytes -- is skipped and never dereferenced.  A filter byte above 4
 * met on the device counts as 0 (the host has refused such files; the rule only keeps a rewritten stream from mattering).  A destination
 * that is 4-byte aligned with a 4-byte aligned stride is written in words, any other in bytes. */
int ocrvi_png_decode_pages(int device, const void* streams_dev, const int64_t* table_dev, int n_pages, void* dst_base, void* workspace,
                           size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * JPEG encode: replaces the cv2.imwrite at the end of the reference's loop (src/pipeline/pipeline2.py:397-400, and the det-only CLI in
 * src/det/test.py) for baseline JPEG.  The host writes the header; colour conversion, down-sampling, forward DCT, quantisation, Huffman
 * coding, bit packing and byte stuffing run on the device, batched over pages, and only the compressed bytes leave it.  Input is uint8
 * RGB (3 bytes per pixel; cv2's BGR is the caller's business, as for decode) or uint8 grey (1 byte per pixel, a one-component file).
 * Written: SOF0, one interleaved scan, the four Annex K Huffman tables, 4:2:0 or 4:4:4.  Not built: 4:2:2, restart intervals, optimised
 * Huffman tables, progressive files, EXIF or ICC segments.
 * The arithmetic is the library's own definition, stated here; tests/jpegenc_ref.py restates it in NumPy.  It equals libjpeg-turbo's
 * default encoder (PIL's Image.save(..., "JPEG", quality=q, subsampling=2 or 0), which is also what cv2.imwrite links) byte for byte,
 * the whole file -- pinned by tests/golden/jpeg_encode_cases.npz; parity with cv2.imwrite itself is UNPINNED (cv2 absent).  All values
 * are integers and shifts are arithmetic.
 *   tables      Annex K.1 luminance and chrominance; s = 5000 / q (integer) for q < 50, else 200 - 2 q; entry = clamp((std s + 50) / 100, 1, 255)
 *   colour      Y = (19595 R + 38470 G + 7471 B + 32768) >> 16, Cb = (-11059 R - 21709 G + 32768 B + 8388608 + 32767) >> 16,
 *               Cr = (32768 R - 27439 G - 5329 B + 8388608 + 32767) >> 16; a grey page is its own Y
 *   planes      luma H x W; 4:2:0 chroma ceil(H / 2) x ceil(W / 2); a component of h x w samples has ceil(h / 8) x ceil(w / 8) real blocks
 *   4:2:0       chroma[i][j] = (a + b + c + d + bias) >> 2 over the cell of rows 2i, 2i+1 and columns 2j, 2j+1, bias 1 in even and 2 in odd
 *               columns j.  Columns beyond W repeat column W - 1 at full resolution, before the down-sampling; so does the one row an
 *               odd H lacks.  Chroma rows beyond ceil(H / 2) repeat the last down-sampled row (not a down-sampling of repeated rows)
 *   4:4:4, grey samples beyond the image repeat the last column and the last row
 *   forward DCT the 8 x 8 "slow integer" form on sample - 128, the LL&M factorisation with the 13-bit constants of the decoder above.
 *               t0..t7 = d0 + d7, d1 + d6, d2 + d5, d3 + d4, d3 - d4, d2 - d5, d1 - d6, d0 - d7; t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2,
 *               t12 = t1 - t2; z1 = (t12 + t13) 4433, out2 = z1 + t13 6270, out6 = z1 - t12 15137; odd part: z1 = t4 + t7, z2 = t5 + t6,
 *               z3 = t4 + t6, z4 = t5 + t7, z5 = (z3 + z4) 9633, out7 = t4 2446 - z1 7373 + (z5 - z3 16069), out5 = t5 16819 - z2 20995 +
 *               (z5 - z4 3196), out3 = t6 25172 - z2 20995 + (z5 - z3 16069), out1 = t7 12299 - z1 7373 + (z5 - z4 3196).
 *               Pass 1 along rows: outputs 0 and 4 are (t10 +- t11) << 2, the others (x + 2^10) >> 11.  Pass 2 down columns: outputs 0 and 4
 *               are (t10 +- t11 + 2) >> 2, the others (x + 2^14) >> 15.  Results are 8 x the true DCT.
 *   quantise    d = 8 x table entry; v = sign(c) ((|c| + (d >> 1)) / d).  AC values are saturated to [-1023, 1023] and DC differences
 *               to [-2047, 2047]: neither is reached from 8-bit samples (|AC| <= about 1020, at coefficient (0, 4) of columns alternating
 *               -128 and 127; |DC| <= 1024), they bound the bits of a block
 *   dummy       in 4:2:0 an MCU may reach past the real luma blocks (an odd number of block columns or rows).  Such a block is not
 *               computed from pixels: its AC coefficients are 0 and its DC is the DC of the block coded just before it in the same MCU;
 *               it takes part in DC prediction like any block
 *   entropy     Annex K.3's four Huffman tables.  DC: the category of the difference to the previous block of the component, then its
 *               low bits (diff - 1 for negatives).  AC in zigzag order: (run, size) symbols, ZRL F0 per 16 zeros of a run, EOB 00 when
 *               coefficient 63 is zero.  The last byte is padded with 1-bits; every FF byte is followed by 00
 *   header      SOI; APP0 JFIF 1.1, units 0, density 1 x 1, no thumbnail; one DQT per table (8-bit, zigzag, ids 0 and 1; grey: id 0 only);
 *               SOF0 (precision 8, height, width, components (1, 0x22 or 0x11, 0) (2, 0x11, 1) (3, 0x11, 1)); one DHT per table in the order
 *               DC0, AC0, DC1, AC1 (grey: DC0, AC0); SOS with Ss = 0, Se = 63, Ah/Al = 0.  After the scan: EOI
 * Block order (of every per-block array below): MCU by MCU in raster order; inside a 4:2:0 MCU the four luma blocks row by row, then
 * Cb, then Cr; 4:4:4: Y, Cb, Cr; grey: block by block.
 * Bound: a block adds at most 1660 bits to the scan -- a DC code of at most 11 bits (chrominance) + 11 low bits, and 63 AC symbols
 * of at most 16 + 10 bits (a ZRL, 11 bits for 16 coefficients, costs less than the coefficients it stands for) -- that is 208 bytes,
 * and byte stuffing at most doubles them: scan_capacity = 2 x 208 x blocks + 16.
 * ------------------------------------------------------------------------------------------------ */
/* Host only.  The two quantisation tables of `quality` (1..100), natural (row-major) order, 64 entries each. */
int ocrvi_jpeg_quant_tables(int quality, uint16_t* luma, uint16_t* chroma);
/* Host only.  Writes a file's header, SOI .. SOS as listed above, into out[0 .. cap); *used = its bytes (at most OCRVI_JPEG_HEADER_MAX;
 * OCRVI_ENOMEM when cap is smaller).  components: 1 (grey) or 3; subsampling: the luma sampling factor, 2 (4:2:0) or 1 (4:4:4), ignored
 * for grey.  The file is header + scan + FF D9. */
#define OCRVI_JPEG_HEADER_MAX 640
int ocrvi_jpeg_encode_header(int width, int height, int components, int subsampling, int quality, void* out, size_t cap, size_t* used);
/* Host only.  For a page's geometry: *blocks = the 8 x 8 blocks of its scan (dummy blocks included), *workspace_bytes = the device bytes
 * ocrvi_jpeg_encode_pages needs for it (a multiple of 256, about 352 per block), *scan_capacity = bytes its stuffed scan never exceeds
 * (the bound above).  offsets (8 values, may be NULL as may the other outputs): the byte offsets of the page's regions in its workspace,
 * for tests and tools -- 0 coef int16 [blocks][64] (quantised, zigzag order; the DC is the block's own value, 0 for a dummy block),
 * 1 dc int16 [blocks] (unset for dummy blocks), 2 DC differences int16 [blocks], 3 bits uint32 [blocks] (what each block adds to the
 * scan), 4 bit offsets uint64 [blocks + 1], 5 the scan before stuffing, 6 FF counts per 4096-byte segment, 7 uint64 the bytes of 5.
 * OCRVI_EINVAL for sides outside 1..65500, other component counts or sampling factors, or more than 20648881 blocks. */
int ocrvi_jpeg_encode_sizes(int width, int height, int components, int subsampling, int64_t* blocks, uint64_t* workspace_bytes,
                            uint64_t* scan_capacity, uint64_t* offsets);
/* Host only.  Fills one entry of the table ocrvi_jpeg_encode_pages reads, int64 [OCRVI_JPEG_ENC_ENTRY]: (0 source offset, 1 source row
 * stride, 2 width, 3 height, 4 components, 5 luma sampling factor, 6 output offset, 7 output capacity, 8 workspace offset, 9 quality,
 * 10..15 zero, 16..47 the two quantisation tables as uint16 [2][64], natural order, 48..63 zero).  Offsets are in bytes from src_base and
 * out_base (signed: pages of one launch may lie in different buffers either side of the base) and from workspace (a multiple of 256);
 * src_stride >= width x components; out_capacity >= scan_capacity. */
#define OCRVI_JPEG_ENC_ENTRY 64
int ocrvi_jpeg_encode_table_entry(int width, int height, int components, int subsampling, int quality, int64_t src_offset, int64_t src_stride,
                                  int64_t out_offset, int64_t out_capacity, int64_t workspace_offset, int64_t* entry);
/* Encodes the scans of n_pages pages in six launches (jpeg_fdct_kernel: pixels -> coefficients and AC bit counts; jpeg_bits_kernel: DC
 * differences, bits per block, their exclusive prefix sum; jpeg_pack_kernel: Huffman codes ORed in at those offsets; jpeg_ffcount_kernel,
 * jpeg_ffscan_kernel, jpeg_stuff_kernel: FF bytes per segment, prefix sum, scatter).  Page i's entropy-coded scan -- the last byte padded
 * with 1-bits, every FF followed by 00, no EOI -- is written at out_base + its output offset and its byte count to lengths_dev[i]
 * (int64; 0 for a skipped page).  table_dev: int64 [n_pages][OCRVI_JPEG_ENC_ENTRY], DEVICE memory like the pixels, read when the kernels
 * run, so a captured graph survives rewritten tables.  Enqueue-only on `stream`: no allocation, no synchronisation.  workspace: 16-byte
 * aligned; the pages' regions of it and of the output must not overlap.  An entry whose fields are out of range, whose regions do not
 * fit workspace_bytes or whose capacity is below scan_capacity is skipped and never dereferenced.  The bytes are the same on every run
 * (integer arithmetic; the only atomics are ORs into zeroed words). */
int ocrvi_jpeg_encode_pages(int device, const void* src_base, const int64_t* table_dev, int n_pages, void* out_base, int64_t* lengths_dev,
                            void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * PNG encode: the lossless way out of the device -- pages for the readers that take .png (DetectionDataset, the reference's recognition
 * loader, src/rec2/dataloader.py:188), annotated pages whose thin outlines JPEG rings around, crops saved for labelling.  Row filtering,
 * deflate, Adler-32, CRC-32 and the assembly of the file all run on the device, batched over pages; only the file's bytes leave it.
 * Input is uint8 RGB (3 bytes per pixel) or uint8 grey (1 byte per pixel).  Written: bit depth 8, colour type 2 or 0, no interlace, and
 * exactly the chunks IHDR, one IDAT, IEND.  Not built: palette, 16-bit or alpha output, Adam7, ancillary chunks, detection of R = G = B.
 * The arithmetic is the library's own definition, stated here; tests/pngenc_ref.py restates it in NumPy.  Any inflater reads the result
 * (zlib, PIL and ocrvi_png_parse are pinned by the tests); no other encoder writes the same bytes.  All values are integers.
 *   filters     bpp = components; x = the raw byte, a = the raw byte bpp to the left, b = the raw byte above, c = the raw byte above-left
 *               (each 0 outside the row or the image: the predictors are raw neighbours, so rows are independent); filtered byte =
 *               (x - p) & 255 with p = 0, a, b, (a + b) >> 1 or Paeth(a, b, c) (as under "PNG decode") for filters 0 .. 4
 *   adaptive    libpng's heuristic: the cost of a filter is the sum of min(v, 256 - v) over the row's filtered bytes (the filter byte is
 *               not counted); the smallest cost wins, ties go to the lower filter number.  A fixed mode gives every row that filter
 *   stream      height x (1 + row_bytes) bytes, every row led by its filter byte; row_bytes = width x components
 *   deflate     the strategy zlib calls Z_RLE: matches at distance 1 only, every block with the cheapest of the three codings.  The
 *               stream is cut into blocks of OCRVI_PNG_ENC_BLOCK bytes (the last may be shorter); no match crosses a block's end
 *   eq          eq[i] = i > 0 and s[i] == s[i - 1] over the whole page stream.  Inside a block a RUN is a maximal set of consecutive
 *               positions with eq = 1; it ends where the block ends, and a block whose first byte has eq = 1 begins with a run (whose
 *               matches reach back into the previous block, whatever its type)
 *   tokens      a byte with eq = 0 is a literal.  A run of L bytes is floor(L / 258) matches of length 258, then its remainder r = L mod
 *               258: one match of length r when r >= 3, else r literals.  Every match has distance 1
 *   counts      per block, of the literal / length symbols 0..285 (RFC 1951, 3.2.5); the end-of-block symbol 256 is counted once
 *   code        lengths from counts, by Huffman's algorithm and a deterministic overflow repair: a symbol of count 0 gets length 0; when
 *               fewer than two symbols have a count, the lowest-numbered symbols of count 0 are given count 1 until two have; the m used
 *               symbols are sorted by (count, symbol) ascending; the tree is built from two queues (the sorted leaves, and the internal
 *               nodes in the order they are made), always taking the lighter head and the leaf on a tie; n[l] = the leaves at depth l,
 *               depths above the limit counted at the limit; while the sum of n[l] 2^(limit - l) exceeds 2^limit: n[limit] -= 1, then for
 *               the largest l < limit with n[l] > 0: n[l] -= 1 and n[l + 1] += 2; finally the lengths are dealt out along the sorted list:
 *               the first n[limit] symbols get the limit, the next n[limit - 1] get limit - 1, and so on.  The code is complete (its
 *               Kraft sum is exactly 1) and canonical (RFC 1951, 3.2.2).  Limit 15 for the literal / length code, 7 for the code-length
 *               code.  The distance code of a dynamic block is always symbols 0 and 1 at one bit each (complete; HDIST = 2)
 *   dynamic     HLIT = max(257, 1 + the last literal / length symbol of non-zero length).  The HLIT + 2 lengths, taken as one sequence,
 *               are cut into maximal runs of equal values.  A run of zeros: repeatedly c = min(left, 138): symbol 18 (c - 11 in 7 bits)
 *               when c >= 11, symbol 17 (c - 3 in 3 bits) when c >= 3, else c symbols 0.  A run of v > 0: symbol v, then while at least 3
 *               are left c = min(left, 6): symbol 16 (c - 3 in 2 bits), then the rest as symbols v.  The code-length code is built from
 *               the counts of these symbols; HCLEN = max(4, 1 + the last position of non-zero length in the order 16 17 18 0 8 7 9 6 10 5
 *               11 4 12 3 13 2 14 1 15)
 *   block type  the bits of a block as stored (3 + the padding to a byte boundary after those 3 bits at the block's position + 32 +
 *               8 n), fixed (3 + the tokens and the end-of-block symbol in RFC 1951's fixed codes, a match costing its length code, its
 *               extra bits and 5) and dynamic (3 + 14 + 3 HCLEN + the code-length symbols with their extra bits + the tokens and the
 *               end-of-block symbol, a match costing its length code, its extra bits and 1); the smallest wins, ties go to the earlier of
 *               stored, fixed, dynamic.  The last block carries BFINAL
 *   checksums   Adler-32 of the stream from per-block partials (A = the sum of the block's n bytes, B = the sum of (n - i) x byte i,
 *               both mod 65521): s2 = (s2 + n s1 + B) mod 65521, then s1 = (s1 + A) mod 65521, from s1 = 1, s2 = 0.  CRC-32 of IDAT's type
 *               and data from raw partials (register 0 at the start, nothing inverted, the first four bytes of the type inverted instead)
 *               of the file's 4096-byte segments [4096 k, 4096 (k + 1)), each multiplied by x^(8 x the bytes that follow it) mod the CRC
 *               polynomial, XORed, inverted
 *   file        the signature; IHDR (width, height, 8, colour type 2 or 0, 0, 0, 0); IDAT = 78 01, the blocks, the Adler-32; IEND
 * Bound: a block never takes more bits than as stored, and a stored block ends on a byte boundary, so
 * file <= 33 + 12 + 2 + sum over blocks (5 + block bytes) + 4 + 12 = 63 + 5 blocks + stream bytes: the output capacity.
 * ------------------------------------------------------------------------------------------------ */
#define OCRVI_PNG_ENC_BLOCK 16384
#define OCRVI_PNG_FILTER_ADAPTIVE 5        /* filter modes: 0 none, 1 sub, 2 up, 3 average, 4 paeth on every row; 5 adaptive */
/* Host only.  For a page's geometry: *stream_bytes = height x (1 + width x components), *blocks = its deflate blocks, *workspace_bytes =
 * the device bytes ocrvi_png_encode_pages needs for it (a multiple of 256, about 1.13 x the stream), *out_capacity = bytes its file never
 * exceeds (the bound above).  offsets (9 values, may be NULL as may the other outputs): the byte offsets of the page's regions in its
 * workspace, for tests and tools -- 0 the filter of every row uint8 [height]; 1 the filtered stream; 2 histograms uint32 [blocks][288]
 * (0..285 the counts, 286 the matches, 287 zero); 3 code lengths uint8 [blocks][320] (0..285 literal / length, 288..306 the code-length
 * code by symbol, the rest zero; filled for every block, whatever its type); 4 the code-length symbols uint16 [blocks][320] (symbol |
 * extra value << 8, zero beyond their count); 5 block records uint32 [blocks][8]: (0 bytes, 1 bits as fixed, 2 bits as dynamic, 3 HLIT,
 * 4 HCLEN, 5 the count of code-length symbols, 6 the type 0 stored 1 fixed 2 dynamic, 7 Adler partials A | B << 16); 6 bit offsets of the
 * blocks from the first bit of the deflate data, uint64 [blocks + 1]; 7 raw CRC partials uint32, one per 4096-byte segment of the file
 * from segment 0 (the one IDAT's type lies in); 8 uint64 [4]: the deflate data's bytes, the Adler-32, the CRC-32, the file's bytes.
 * OCRVI_EINVAL for sides outside 1..65500, other component counts, or a page whose IDAT could exceed 2^31 - 1 bytes. */
int ocrvi_png_encode_sizes(int width, int height, int components, uint64_t* stream_bytes, int64_t* blocks, uint64_t* workspace_bytes,
                           uint64_t* out_capacity, uint64_t* offsets);
/* Host only.  Fills one entry of the table ocrvi_png_encode_pages reads, int64 [OCRVI_PNG_ENC_ENTRY]: (0 source offset, 1 source row
 * stride, 2 width, 3 height, 4 components, 5 filter mode, 6 output offset, 7 output capacity, 8 workspace offset, 9..15 zero).  Offsets
 * are in bytes from src_base and out_base (signed; the output offset a multiple of 16) and from workspace (a multiple of 256);
 * src_stride >= width x components; out_capacity >= the output capacity. */
#define OCRVI_PNG_ENC_ENTRY 16
int ocrvi_png_encode_table_entry(int width, int height, int components, int filter, int64_t src_offset, int64_t src_stride, int64_t out_offset,
                                 int64_t out_capacity, int64_t workspace_offset, int64_t* entry);
/* Encodes n_pages pages in six launches (png_filter_kernel: filters, costs, the filtered stream; png_analyse_kernel: tokens, counts,
 * both codes and the bits of every block; png_scan_kernel: block types, bit offsets, Adler-32, the file's first 43 bytes;
 * png_pack_kernel: the blocks ORed in at those offsets; png_crc_kernel, png_finish_kernel: CRC-32, IEND).  Page i's whole file is
 * written at out_base + its output offset and its byte count to lengths_dev[i] (int64; 0 for a skipped page).  table_dev: int64
 * [n_pages][OCRVI_PNG_ENC_ENTRY], DEVICE memory like the pixels, read when the kernels run, so a captured graph survives rewritten
 * tables.  Enqueue-only on `stream`: no allocation, no synchronisation.  workspace and out_base: 16-byte aligned; the pages' regions of
 * them must not overlap.  An entry whose fields are out of range, whose regions do not fit workspace_bytes or whose capacity is below the
 * output capacity is skipped and never dereferenced.  Source rows may be src_stride apart.  The host builds no code and sees no
 * histogram.  The bytes are the same on every run (integer arithmetic; the atomics are adds into LDS histograms and ORs into zeroed
 * words). */
int ocrvi_png_encode_pages(int device, const void* src_base, const int64_t* table_dev, int n_pages, void* out_base, int64_t* lengths_dev,
                           void* workspace, size_t workspace_bytes, void* stream);
/* Test hook: runs the device's code-construction routine ("code" above) on n_codes histograms of n_symbols (2..288) counts each, uint32
 * [n_codes][n_symbols] in DEVICE memory (every histogram's counts must sum below 2^32), with the length limit `limit` (1..15, n_symbols
 * <= 2^limit); lengths_dev: uint8 [n_codes][n_symbols].  Enqueue-only on `stream`. */
int ocrvi_test_png_code_lengths(int device, const uint32_t* counts_dev, int n_codes, int n_symbols, int limit, uint8_t* lengths_dev, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Result overlay: the page `--save_result` writes.  Replaces draw_boxes_with_text (src/pipeline/pipeline2.py:173-190) as the per-image
 * loop calls it (:358-360) ahead of cv2.imwrite (:397-400): every box outlined, its 1-based index written beside it.  cv2.drawContours
 * and cv2.putText are not reproduced (cv2 and its Hershey glyphs are absent from the build container; its thick lines are fixed-point
 * convex fills): the rule below is the library's own, exact on integers, and parity with cv2 is UNPINNED.  tests/overlay_ref.py restates
 * the rule in numpy int64 and in fractions.
 *
 * THE PAINTING RULE.  Everything painted is a list of segments with integer endpoints; segment number s (its ORDINAL, the position in
 * the list) has a colour and a thickness T, 1 <= T <= 15.  Pixel (x, y) is its integer centre p.  For segment a -> b:
 *     d = b - a,  L2 = d.d,  t = (p - a).d
 *     t <= 0   (this includes a == b)   covered iff 4 |p - a|^2 <= T^2
 *     t >= L2                           covered iff 4 |p - b|^2 <= T^2
 *     otherwise, c = d.x (p - a).y - d.y (p - a).x:   covered iff c^2 <= floor(T^2 L2 / 4)
 * (the last line is 4 dist^2 <= T^2 without the factor that would overflow).  A pixel no segment covers keeps its value and is not
 * written.  A pixel several segments cover takes the colour of the one with the LARGEST ordinal -- the reference's sequential overdraw,
 * independent of evaluation order: the kernel needs neither atomics on global memory nor an order between workgroups.
 * Limits: page sides 1..16384, every endpoint (labels included) in [-16384, 16384]; all products then stay below 2^63 in int64.
 * Anything else is OCRVI_EINVAL.  Endpoints outside the page are legal.  Hand check: (2,5) -> (8,5) with T = 2 paints
 * {2 <= x <= 8, 4 <= y <= 6} and (1,5), (9,5): 23 pixels.
 *
 * THE SEGMENT ORDER.  For pair i = 0, 1, .. of a page (box i with its text; the strings themselves are never rendered, as in the
 * reference, which writes str(idx + 1)):
 *   1. the n_i closed edges v_k -> v_(k+1 mod n_i) of the box in the box colour (one vertex: one zero-length edge, a disc; two vertices:
 *      the edge there and back).  A box without vertices contributes nothing, neither outline nor label; it keeps its index.
 *   2. the label: top = the FIRST vertex of minimum y; text_pos = (top.x, top.y - 10); if text_pos.y < 20 then text_pos = (top.x, max_y +
 *      20) with max_y the largest vertex y (pipeline2.py:182-187).  The decimal digits of i + 1, left to right, digit k with its origin at
 *      (text_pos.x + 10 k, text_pos.y) (bottom-left, as cv2.putText), each as the strokes of a seven-stroke font, in the order A..G, in the
 *      label colour and the same thickness:
 *          A (0,-10)-(6,-10)  B (6,-10)-(6,-5)  C (6,-5)-(6,0)  D (0,0)-(6,0)  E (0,-5)-(0,0)  F (0,-10)-(0,-5)  G (0,-5)-(6,-5)
 *          0 ABCDEF  1 BC  2 ABDEG  3 ABCDG  4 BCFG  5 ACDFG  6 ACDEFG  7 ABC  8 ABCDEFG  9 ABCDFG        (csrc/overlay_font.h)
 * ------------------------------------------------------------------------------------------------ */
#define OCRVI_OVERLAY_SEG 8        /* int32 fields of a segment: (a.x, a.y, b.x, b.y, colour = r | g << 8 | b << 16, T, pair index i, 0) */
#define OCRVI_OVERLAY_PRIM 8       /* int32 fields of a primitive: (first segment, one past its last segment, x0, y0, x1, y1, kind, pair index i) */
#define OCRVI_OVERLAY_MAX_COORD 16384
/* Host only, needs no GPU.  Builds the segment table and the primitive table of n_pages pages.
 *   points int32 [total][2], offs int32 [n_boxes + 1]: box j = points[offs[j] .. offs[j+1]) (the convention of ocrvi_min_area_quads);
 *   page_boxes int32 [n_pages + 1]: page p owns boxes page_boxes[p] .. page_boxes[p+1]; page_pairs int32 [n_pages] or NULL: the number of
 *   texts of page p -- only min(boxes, texts) pairs are drawn, as zip() does (NULL: every box); page_hw int32 [n_pages][2] = (h, w);
 *   box_rgb, label_rgb: r | g << 8 | b << 16; thickness: T.
 * A primitive is one box outline (kind 0) or one label (kind 1): its range of the segment table and the inclusive bounding box of its
 * endpoints dilated by ceil(T / 2) on every side.  Primitives and segments are listed page by page in drawing order; prim_offs int32
 * [n_pages + 1]: page p owns primitives prim_offs[p] .. prim_offs[p+1].  Segment numbers are indices into the one table of all pages.
 * Sizes: *n_segs and *n_prims are always written; with segs, prims and prim_offs all NULL nothing else is (the size query; validation
 * still runs).  Never more than sum n_i + 7 digits(i + 1) segments and two primitives per pair.  seg_cap / prim_cap: entries the
 * tables hold.
 * OCRVI_EINVAL with a message, nothing painted anywhere: a null pointer, n_pages < 0, a page side outside 1..16384, T outside 1..15, a
 * colour above 0xffffff, offsets that run backwards, a vertex or a label endpoint outside [-16384, 16384], a table too small. */
int ocrvi_overlay_segments(const int32_t* points, const int32_t* offs, const int32_t* page_boxes, const int32_t* page_pairs,
                           const int32_t* page_hw /*[n_pages][2]*/, int n_pages, uint32_t box_rgb, uint32_t label_rgb, int thickness,
                           int32_t* segs /*[seg_cap][OCRVI_OVERLAY_SEG]*/, int64_t seg_cap, int32_t* prims /*[prim_cap][OCRVI_OVERLAY_PRIM]*/,
                           int64_t prim_cap, int32_t* prim_offs /*[n_pages + 1]*/, int64_t* n_segs, int64_t* n_prims);
/* Paints n_pages pages IN PLACE in one launch (pipeline2.py:173-190 by the rule above).  pages: a page table (OCRVI_PAGE_ENTRY) of uint8
 * HWC [h,w,3] pages; prims, segs, prim_offs: the tables of ocrvi_overlay_segments for the same pages, all in DEVICE memory; max_h, max_w:
 * at least every page's height and width (they size the grid; 1..16384).  1 <= n_pages <= 65535.  Enqueue-only on `stream`: no
 * allocation, no synchronisation; tables and pages are read when the kernel runs.  An invalid page entry is skipped and never
 * dereferenced.  One workgroup per 64 x 16 tile: the page's primitive boxes are tested against the tile and the hits compacted in LDS, a
 * tile without a hit ends there without touching the page; the hit primitives' segments are staged through LDS 256 at a time (those
 * whose own dilated box misses the tile are dropped while staging) and every thread keeps, for its four pixels, the largest covering
 * ordinal; only covered pixels are stored.  The result does not depend on the order of evaluation. */
int ocrvi_overlay_pages(int device, const int64_t* pages, int n_pages, const int32_t* prims, const int32_t* segs, const int32_t* prim_offs,
                        int max_h, int max_w, void* stream);

/* Replaces DBPostProcessor(thresh, box_thresh, max_candidates, unclip_ratio).__call__ with .min_area (src/det/test.py:46-106) on a HOST
 * probability map prob[H*W] (the reference also runs this stage on the CPU after `.cpu().numpy()`, pipeline2.py:320-321).
 * Output: the unclipped polygons as int32 (x, y) pairs in points[2*cap_points]; box i owns points box_offsets[i] .. box_offsets[i+1]
 * (box_offsets has cap_boxes+1 entries); scores[i] is its box_score_fast value; *n_boxes the number of boxes, in the reference's order. */
int ocrvi_db_postprocess(const float* prob, int H, int W, float thresh, float box_thresh, int max_candidates, float unclip_ratio,
                         float min_area, int32_t* points, int cap_points, int32_t* box_offsets, float* scores, int cap_boxes, int* n_boxes);

/* Replaces unclip()'s Clipper call for a given offset distance (src/det/test.py:37-43: PyclipperOffset().AddPath(box, JT_ROUND,
 * ET_CLOSEDPOLYGON); Execute(distance)[0]): pts int32 (x, y) pairs of a closed polygon -> the offset polygon after Clipper's closing
 * union (raw round-join offset path, then the outline of its positive-winding region), int32 pairs in out[2*cap_pts]; *n_out points
 * (0 when the input degenerates).  Host code; ocrvi_db_postprocess calls the same routine with distance = area * unclip_ratio / length. */
int ocrvi_unclip_polygon(const int32_t* pts, int n_pts, double distance, int32_t* out, int cap_pts, int* n_out);

/* Replaces the host middle of the per-image loop for a batch of pages (src/pipeline/pipeline2.py:320-343): post_processor(prob_map)
 * (src/det/test.py:55-106) on each of the n_pages host maps prob[n_pages][H][W] -> boxes divided by (scale_w, scale_h) with the int64
 * truncation of pipeline2.py:324-328 -> crop_image's clamped bounding rectangle in the orig_h x orig_w page (src/det/test.py:123-130).
 * rects[(page * cap_per_page + i) * 5] = (page_base + page, x, y, w, h) -- the layout ocrvi_crop_resize_normalize consumes --,
 * scores (may be NULL) likewise, counts[page] = boxes of that page.  Pages are independent and run on `threads` host threads. */
int ocrvi_db_boxes_batch(const float* prob, int n_pages, int H, int W, float thresh, float box_thresh, int max_candidates,
                         float unclip_ratio, float min_area, double scale_w, double scale_h, int orig_h, int orig_w, int page_base,
                         int32_t* rects, float* scores, int cap_per_page, int32_t* counts, int threads);

/* ocrvi_db_boxes_batch for pages of different original sizes that share one detector shape (the per-image loop of pipeline2.py:306-343
 * over a bucket of pages): page p's boxes are divided by (scale_w[p], scale_h[p]) = (new_w/w, new_h/h) with the int64 truncation of
 * pipeline2.py:324-328 and clamped to its orig_h[p] x orig_w[p] page.  Per page p, besides rects (first column = page_ids[p]), scores and
 * counts as ocrvi_db_boxes_batch writes them:
 *   points      int32 [n_pages][cap_points][2]      the rescaled polygons (what rescale_boxes returns), box after box
 *   box_offsets int32 [n_pages][cap_per_page + 1]   box i of page p owns points box_offsets[p][i] .. box_offsets[p][i+1] of its page row
 *   overflow    int32 [n_pages]                     0, or the number of polygon points page p needs when that exceeds cap_points: its
 *                                                   points and offsets are then not written (rects, scores and counts are) and the
 *                                                   caller redoes the page alone with room for them.  No page is truncated.
 * Runs on the same host thread pool as ocrvi_db_boxes_batch. */
int ocrvi_db_boxes_pages(const float* prob, int n_pages, int H, int W, float thresh, float box_thresh, int max_candidates, float unclip_ratio,
                         float min_area, const double* scale_w, const double* scale_h, const int32_t* orig_h, const int32_t* orig_w,
                         const int32_t* page_ids, int32_t* points, int cap_points, int32_t* box_offsets, int32_t* rects, float* scores,
                         int cap_per_page, int32_t* counts, int32_t* overflow, int threads);

/* Device half of the same stage (the reference thresholds on the host, `pred[0] > self.thresh`, src/det/test.py:57,
 * after copying the whole map, pipeline2.py:320).  prob: DEVICE float32 [n_pages,H,W] (W % 32 == 0).  Outputs, all DEVICE buffers:
 *   mask_bits  uint32 [n_pages,H,W/32]   bit (x & 31) of word (x >> 5) = prob > thresh
 *   comps      int32  [n_pages,cap,8]    per 8-connected component: x0, y0, x1, y1 (inclusive box), pixel count, root (index y*W+x of
 *                                        its first pixel in raster order), sum of round(prob * 2^20) as uint64 in ints 6..7; row order
 *                                        is arbitrary (sort by root for a canonical order)
 *   counts     int32  [n_pages]          components found (may exceed cap: rows beyond cap are not written)
 *   offsets    int64  [n_pages,cap+1]    start, in floats, of each component's box inside the page's packed region; [min(count,cap)] = total
 *   packed     float32[n_pages,pack_cap] the probability values inside the component boxes, row-major per box, back to back (left
 *                                        unwritten for a page whose total exceeds pack_cap).  offsets and packed may both be NULL.
 * workspace: ocrvi_db_components_workspace_bytes(n_pages, H, W) bytes of device memory.  Asynchronous on `stream`. */
size_t ocrvi_db_components_workspace_bytes(int n_pages, int H, int W);
int ocrvi_db_components(int device, const float* prob, int n_pages, int H, int W, float thresh, uint32_t* mask_bits, int32_t* comps,
                        int32_t* counts, int cap, long long* offsets, float* packed, long long pack_cap, void* workspace, void* stream);
/* ocrvi_db_boxes_batch fed by HOST copies of ocrvi_db_components' outputs instead of the full maps: same results (the segmentation comes
 * from mask_bits, the map is rebuilt inside the component boxes only, which is all box_score_fast reads).  skipped[page] = 1 (and
 * counts[page] = 0) for a page whose table or boxes overflowed (count > cap or total > pack_cap): process that page from its full map. */
int ocrvi_db_boxes_batch_sparse(const uint32_t* mask_bits, const int32_t* comps, const int32_t* comp_counts, int cap, const long long* offsets,
                                const float* packed, long long pack_cap, int n_pages, int H, int W, float box_thresh, int max_candidates,
                                float unclip_ratio, float min_area, double scale_w, double scale_h, int orig_h, int orig_w, int page_base,
                                int32_t* rects, float* scores, int cap_per_page, int32_t* counts, int threads, int32_t* skipped);

/* ------------------------------------------------------------------------------------------------
 * DB ground truth: the reference's DetectionDataset without augmentation (src/det/dataloader.py:27-362, is_training=False, plus the
 * threshold maps of is_training=True on request) -- `image`, `gt`, `mask`, `thresh_map`, `thresh_mask` from polygon annotations.
 * The reference builds them on the host with shapely, pyclipper and cv2; here the polygon geometry runs on the host (Clipper's offset
 * is host code in this library already) and every pixel is produced on the device.  Parity with GEOS, Clipper and cv2 is unpinned, as
 * for the rest of the host geometry; tests/dbtarget_ref.py states the same path in Python and the library equals it exactly.
 * ------------------------------------------------------------------------------------------------ */
#define OCRVI_DB_TARGET_GT 0      /* fill gt with 1                                  (cv2.fillPoly(gt, [shrunk], 1.0), :342) */
#define OCRVI_DB_TARGET_MASK 1    /* fill mask with 0                                (cv2.fillPoly(mask, [polygon], 0.0), :344) */
#define OCRVI_DB_TARGET_THRESH 2  /* fill thresh_mask with 1, thresh_map with thresh_max  (_draw_border_map, :164-194) */
#define OCRVI_DB_TARGET_JOB 8     /* int32 fields of a job: (image, kind, p0, p1, x0, y0, x1, y1): points p0 .. p1-1, their inclusive bounding box */
#define OCRVI_DB_TARGET_MAX_SIDE 16384   /* largest image side and S: keeps every coordinate below 2^20, where the integer fill tests
                                          * decide as the double arithmetic of the stated fill rule does */
/* Replaces the polygon loop of _load_sample (dataloader.py:334-350) with _shrink_polygon (:71-102), _dilate_polygon (:104-133) and the
 * gates of _draw_border_map (:139-161) for n_images images.  HOST code.  Inputs: sizes int32 [n_images][2] = (h, w); xy float32 (x, y)
 * pairs of every vertex; polygon k owns vertices poly_offsets[k] .. poly_offsets[k+1]; image i owns polygons image_offsets[i] ..
 * image_offsets[i+1] (both start at 0).  Coordinates must be finite; a polygon of fewer than 3 vertices is skipped (:320).
 * Per polygon, in the reference's order:
 *   1. clip to [0, w-1] x [0, h-1] in float32 (:336-337);
 *   2. shapely is_valid / .area / .length on the FLOAT ring, stated here as: all in double without fused multiply-adds; consecutive
 *      duplicate vertices are dropped, at least 3 must remain; a predicate is the sign of (bx-ax)(cy-ay) - (by-ay)(cx-ax); two edges
 *      that are not neighbours may not share a point (touching counts), two neighbours may share only their common vertex (the ring is
 *      simple); area = |sequential shoelace sum| / 2 and length = sequential sum of sqrt(dx dx + dy dy) over the ring as given;
 *   3. `not valid or area < 1` or `length < 1` -> no shrunk polygon;
 *   4. d = area * (1 - shrink_ratio^2) / length;  5. the vertices truncated (astype(int));
 *   6. Execute(-d): the raw round-join offset path at -d, then EVERY outer loop of its positive-winding region (a shrink can fall apart);
 *   7. no loop -> a MASK job with the truncated polygon;  8. else a GT job with the loop of largest signed area -- among equal areas
 *      the loop whose smallest vertex (by x, then y) is smallest, then the first found;
 *   9. with want_thresh, a valid polygon and d >= 1: Execute(+d) (ocrvi_unclip_polygon's routine) -> a THRESH job when it is not empty.
 * A FINDING about the reference, reproduced and not corrected: _draw_border_map takes np.minimum(dist_inside, dist_outside) (:172-177),
 * and one of the two is 0 at every pixel, so its threshold map is float32(thresh_max) over the whole dilated polygon and thresh_min is
 * never used.  A THRESH job is therefore a plain fill; no distance transform is involved.
 * Outputs: jobs int32 [cap_jobs][OCRVI_DB_TARGET_JOB] and points int32 [cap_points][2], image after image, polygon after polygon, the
 * GT or MASK job of a polygon before its THRESH job; *n_jobs, *n_points = the room needed.  When either exceeds its capacity *overflow = 1
 * and nothing is written (call again with that room), otherwise 0.  Nothing is ever truncated.  Images run on `threads` host threads,
 * the pool of ocrvi_db_boxes_batch. */
int ocrvi_db_target_jobs(const int32_t* sizes, const float* xy, const int32_t* poly_offsets, const int32_t* image_offsets, int n_images,
                         double shrink_ratio, int want_thresh, int32_t* jobs, int cap_jobs, int32_t* points, int cap_points, int32_t* n_jobs,
                         int32_t* n_points, int32_t* overflow, int threads);
/* Replaces the four maps of _load_sample (:328-332, the cv2.fillPoly calls :342, :344, :164-194) after _resize_pad (:263-271).  jobs, points:
 * DEVICE copies of ocrvi_db_target_jobs' output; rows DEVICE int32 [n][4] = (h, w, new_h, new_w) with (new_h, new_w) = (int(h * scale),
 * int(w * scale)), scale = S / max(h, w) (:242-244).  Writes float32 [n,1,S,S]: gt = 0 with the GT fills, mask = 1 inside new_h x new_w with
 * the MASK fills at 0, thresh_map / thresh_mask = 0 with the THRESH fills (thresh_max, 1); 0 in the pad.  A row with new_h <= 0 or
 * new_w <= 0 gives four zero maps (the reference's _blank_sample: cv2.resize raises).
 * The fill rule is this library's statement of cv2.fillPoly: the pixels of the 8-connected Bresenham line (cv::LineIterator) from vertex i
 * to vertex i+1 of every edge, plus the even-odd interior at pixel centres with the half-open vertex rule (row y meets edge a-b when
 * ay <= y < by or by <= y < ay; crossings sorted and paired; x filled for ceil(lo) <= x <= floor(hi)).  The maps are filled at h x w and then
 * sampled as cv2.resize(INTER_NEAREST) does: output (X, Y) takes source (sx, sy), sx = min(floor(X * (1.0 / (new_w / w))), w - 1) in
 * double, likewise sy (for scale == 1.0 that is the identity, the reference's copy).  Jobs may overlap and run in any order: every store
 * to a map writes that map's constant.  A job whose image or point range is out of bounds is skipped.  Enqueue-only on `stream`, no
 * allocation, no workspace. */
int ocrvi_db_target_maps(int device, const int32_t* jobs, int n_jobs, const int32_t* points, int n_points, const int32_t* rows, int n, int S,
                         float thresh_max, float* gt, float* mask, float* thresh_map, float* thresh_mask, void* stream);
/* Replaces _resize_pad's image half (:240-261): page i of the page table (OCRVI_PAGE_ENTRY) resized to rows[i]'s (new_h, new_w) with
 * ocrvi_resize_u8's arithmetic (the identity when the sizes agree: the scale == 1.0 branch), normalised in FLOAT32 -- ((v / 255) - mean)
 * / std with float32 mean and std, every step rounded to float32 (:251-252), not the float64 form of ocrvi_normalize_u8 -- and
 * zero-padded to S x S: out float32 [n,3,S,S].  An invalid page entry or a row with new_h <= 0 or new_w <= 0 gives zeros.
 * Enqueue-only on `stream`. */
int ocrvi_resize_normalize_pad_pages(int device, const int64_t* pages, const int32_t* rows, int n, int S, float* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Validation: the numbers the reference's two validation loops report (src/det/val.py, src/rec2/val.py) from maps, log-probs and ids
 * that stay on the device.  Forward values only: no backward pass, no SGM term (both are training).  All three
 * entries are enqueue-only on `stream`, allocate nothing and never synchronise; every pointer is DEVICE memory.
 * ------------------------------------------------------------------------------------------------ */
/* Replaces DBLoss.forward (model/det/loss.py:70-90, with BalanceCrossEntropyLoss :10-31, DiceLoss :38-50, MaskL1Loss :57-59) and the
 * counts of compute_metrics (src/det/val.py:26-35), up to the final divisions, which are host arithmetic on the record below.
 * Eight float32 maps of n = N*H*W elements ([N,1,H,W]): binary, thresh, thresh_binary, bin_logits as ocrvi_det_forward writes them; gt, mask,
 * thresh_map, thresh_mask from the batch.  No alignment is asked of them (16-byte aligned maps are read four pixels at a time).
 * Per pixel, every term in float32 exactly as the reference forms it:
 *   gm = gt * mask, ngm = (1 - gt) * mask;  p = (int)gm & 255, q = (int)ngm & 255   (`.byte()`: truncation, so a fractional product is 0)
 *   loss = max(x, 0) - x * gt + log1p(exp(-|x|)),  x = bin_logits                   (binary_cross_entropy_with_logits, reduction 'none')
 *   P = (binary > 0.5 ? 1 : 0) * mask;  tp += (P == 1 and gm == 1), fp += (P == 1 and gm == 0), fn += (P == 0 and gm == 1)
 * Record (OCRVI_DET_EVAL_RECORD_BYTES bytes, 8-byte aligned, 13 slots of 8 bytes; slots 0..5 int64, 6..12 float64):
 *   TP, FP, FN        the three counts above
 *   POSITIVES         sum p            NEGATIVES  sum q
 *   K                 negative_count = min(NEGATIVES, (int64)trunc((double)POSITIVES * negative_ratio)), formed on the device; 0 when the
 *                     product is below 1 or NaN
 *   POS_BCE           sum loss * p
 *   TOPK_BCE          sum of the K largest values of loss * q over all pixels (torch.topk(negative_loss.view(-1), negative_count).sum());
 *                     0 when K = 0
 *   DICE_INTER        sum (thresh_binary * gt) * mask     PRED_MASK  sum thresh_binary * mask     GT_MASK  sum gm
 *   L1_NUM            sum |thresh - thresh_map| * thresh_mask        THRESH_MASK  sum thresh_mask
 * so that, with eps = 1e-6:  l_prob = (POS_BCE + TOPK_BCE) / (POSITIVES + K + eps),  l_binary = 1 - 2 DICE_INTER / (PRED_MASK + GT_MASK + eps),
 * l_thresh = L1_NUM / (THRESH_MASK + eps),  loss = l_prob + alpha l_binary + beta l_thresh.
 * Sums: each float32 term is widened to float64 and added in float64, per thread, then per wave, per block and over the blocks in index
 * order; the grid is a function of n alone and the counts are integer atomics, so two runs on the same inputs give the same bits.
 * Top-k: the fused pass also writes loss * q as a 4-byte stream into the workspace.  For gt in [0, 1] the values are non-negative, so
 * their bit patterns order as the values do: a radix select over the 31 bits below the sign (9 + 11 + 11, one LDS histogram pass each, the first inside
 * the fused pass) finds the K-th largest value v, and TOPK_BCE = sum of the values above v + (K - their number) * v, exact whatever the
 * ties.  Zeros are not counted: when fewer than K values are non-zero, v = 0.  Non-finite logits may give NaN or infinite sums (a NaN
 * orders above every number in the select); every pass is a fixed number of steps whatever the data.
 * workspace: 256-byte aligned, ocrvi_det_eval_workspace_bytes(N, H, W, &bytes) bytes (114944 + 4 n rounded up to a multiple of 256); OCRVI_ENOMEM when it is short. */
#define OCRVI_DET_EVAL_RECORD_BYTES 104
#define OCRVI_DET_EVAL_TP 0
#define OCRVI_DET_EVAL_FP 1
#define OCRVI_DET_EVAL_FN 2
#define OCRVI_DET_EVAL_POSITIVES 3
#define OCRVI_DET_EVAL_NEGATIVES 4
#define OCRVI_DET_EVAL_K 5
#define OCRVI_DET_EVAL_POS_BCE 6
#define OCRVI_DET_EVAL_TOPK_BCE 7
#define OCRVI_DET_EVAL_DICE_INTER 8
#define OCRVI_DET_EVAL_PRED_MASK 9
#define OCRVI_DET_EVAL_GT_MASK 10
#define OCRVI_DET_EVAL_L1_NUM 11
#define OCRVI_DET_EVAL_THRESH_MASK 12
int ocrvi_det_eval_workspace_bytes(int N, int H, int W, size_t* bytes);
int ocrvi_det_eval(int device, const float* binary, const float* thresh, const float* thresh_binary, const float* bin_logits,
                   const float* gt, const float* mask, const float* thresh_map, const float* thresh_mask, int N, int H, int W,
                   double negative_ratio, void* record, void* workspace, size_t workspace_bytes, void* stream);

/* Replaces nn.CTCLoss(blank, reduction='none') as SVTRv2Loss.forward calls it (model/rec2/loss.py:44-63), before zero_infinity and the
 * reduction, which are host arithmetic on B numbers.  log_probs float32 [T,B,C], exactly what ocrvi_rec_forward writes; targets int32
 * [B,Lmax] (row b holds target_lengths[b] labels, the rest is never read; the reference's flattening, loss.py:57-61, is not needed);
 * target_lengths int32 [B]; input_lengths int32 [B] or NULL, which means T for every row; 0 <= blank < C; Lmax <=
 * OCRVI_CTC_LOSS_MAX_TARGET.  nll float64 [B].
 * Row b, with L = target_lengths[b], Tb = input_lengths[b]: the extended sequence l' has S = 2L + 1 states, blank at the even ones and
 * label (s - 1) / 2 at the odd ones.  In float64 log space, from the float32 log-probs y:
 *   alpha_0(0) = y[0,b,blank], alpha_0(1) = y[0,b,l'_1], alpha_0(s) = -inf otherwise
 *   alpha_t(s) = logsumexp(alpha_{t-1}(s), alpha_{t-1}(s-1), alpha_{t-1}(s-2) if s is odd, s >= 3 and l'_s != l'_{s-2}) + y[t,b,l'_s]
 *   nll[b] = -logsumexp(alpha_{Tb-1}(S-1), alpha_{Tb-1}(S-2))
 * logsumexp subtracts the largest term first and is -inf when every term is.  No alignment of the labels over Tb steps (L plus the
 * number of adjacent repeats exceeds Tb) gives +inf.  Lengths outside [0, Lmax] / [0, T] are clamped into them and a label outside
 * [0, C) has probability 0, so no address outside the buffers is formed; Tb = 0 gives 0 for L = 0 and +inf otherwise.
 * One wave per row: state s in lane s mod 64, the two alpha rows in LDS. */
#define OCRVI_CTC_LOSS_MAX_TARGET 1024
int ocrvi_ctc_loss(int device, const float* log_probs, int T, int B, int C, const int32_t* targets, int Lmax, const int32_t* target_lengths,
                   const int32_t* input_lengths, int blank, double* nll, void* stream);

/* Replaces editdistance.eval(pred, gt) inside compute_cer (src/rec2/val.py:14-24) for B pairs of id rows: dist int32 [B] = the
 * Levenshtein distance (insertion, deletion and substitution cost 1 each) between
 *   the first pred_lens[b] ids of pred_ids [B,T] with every id < 2 dropped -- the ids / lens buffers of ocrvi_rec_forward: the collapse there
 *   drops the blank and keeps pad id 1, Tokenizer.decode drops both (tokenizer.py:73) -- and
 *   the first gt_lens[b] ids of gt_ids [B,G], encoded on the host, a character outside the alphabet as -2: it equals no prediction id,
 *   which is what the string distance does with such a character.
 * Lengths are clamped into [0, T] / [0, G]; T, G <= OCRVI_EDIT_DISTANCE_MAX_LEN.  One wave per pair: a row of the DP (one row per
 * prediction id, one column per ground-truth id) lies across the lanes, 64 columns at a time; with t[j] = min(above + 1, diagonal +
 * (ids differ)) the insertion chain is a prefix minimum, d[j] = j + min over k <= j of (t[k] - k), carried from one group of 64 columns
 * to the next. */
#define OCRVI_EDIT_DISTANCE_MAX_LEN 2048
int ocrvi_edit_distance(int device, const int32_t* pred_ids, int T, const int32_t* pred_lens, const int32_t* gt_ids, int G,
                        const int32_t* gt_lens, int B, int32_t* dist, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Kernel-level test/bench hooks (same kernels the models launch; used by tests/ and bench.py for
 * per-kernel parity and roofline timing).
 * ------------------------------------------------------------------------------------------------ */
/* The 27-channel offset / mask conv of DeformableConv2d alone (dcn.py:42-46: self.offset_conv, then sigmoid on channels 18..26): x float32
 * NCHW [N,C,H,W] (device), weight float32 host [27,C,3,3], bias host [27]; pad 1, stride 1 or 2; out DEVICE float32 [N,Ho,Wo,32]
 * (0..17 offsets, 18..26 mask, 27..31 zero).  Test hook: allocates and synchronises internally. */
int ocrvi_test_offset_conv(int device, int dtype, const float* x, const float* weight_host, const float* bias_host, int N, int C, int H, int W,
                           int stride, float* out, int iters, float* avg_ms);
/* Modulated deformable 3x3 conv, pad 1, dil 1 (torchvision.ops.deform_conv2d as called at dcn.py:48-57) with
 * a fused per-channel bias (+ optional ReLU) epilogue.  x float32 NCHW [N,C,H,W]; offset [N,18,Ho,Wo];
 * mask [N,9,Ho,Wo] (already sigmoided); weight float32 host [Co,C,3,3]; bias float32 host [Co] or NULL;
 * out float32 NCHW [N,Co,Ho,Wo].  Allocates and synchronises internally (test hook, not graph-capturable). */
int ocrvi_test_deform_conv(int device, int dtype, const float* x, const float* offset, const float* mask,
                           const float* weight_host, const float* bias_host, int N, int C, int H, int W, int Co,
                           int stride, int relu, float* out, int iters, float* avg_ms);
/* The same with a residual in the epilogue, as conv2 of a BasicBlock in layers 2-4 of the ResNet-18 backbone has it
 * (torchvision.models.resnet.BasicBlock with backbone.py:39-53): out = act(deform_conv2d(x) + bias + res).  res: float32 NCHW
 * [N,Co,Ho,Wo] on the device, converted to NHWC in the compute type exactly as x is (so in the 16-bit modes the kernel reads res rounded
 * to that type). */
int ocrvi_test_deform_conv_res(int device, int dtype, const float* x, const float* offset, const float* mask,
                               const float* weight_host, const float* bias_host, const float* res, int N, int C, int H, int W, int Co,
                               int stride, int relu, float* out, int iters, float* avg_ms);
/* ocrvi_test_deform_conv_res with res optional (NULL: no residual) and the output buffer owned by the caller: out_raw is a DEVICE buffer
 * of at least N*Ho*Wo rows of Co `dtype` elements (NHWC) that the kernel writes directly (the caller pre-fills it, and any rows past the
 * last, and reads the bytes back); only its first N*Ho*Wo rows are converted to out, float32 NCHW [N,Co,Ho,Wo] DEVICE. */
int ocrvi_test_deform_conv_raw(int device, int dtype, const float* x, const float* offset, const float* mask,
                               const float* weight_host, const float* bias_host, const float* res, int N, int C, int H, int W, int Co,
                               int stride, int relu, void* out_raw, float* out);
/* Host-only (no GPU): which kernel the deformable convolution of ocrvi_test_deform_conv takes on a device of n_cu compute units and how
 * it tiles the map, from the same functions the launchers use.  plan = {1: the pipelined kernel (csrc/dcn_pipe.h), 0: conv_gemm's
 * deformable mode; rows of a tile (128; conv_gemm: 32 or 64); columns of a tile (128 or 256); pipelined kernel: log2 of the pixel
 * patch's width, a tile being (128 >> lw) x (1 << lw) output pixels (conv_gemm: 0); tiles; workgroups; most tiles one workgroup walks;
 * K-steps per tile}. */
int ocrvi_test_dcn_plan(int dtype, int N, int C, int H, int W, int Co, int stride, int n_cu, int32_t plan[8]);
/* Plain conv2d (groups, stride (sh,sw), square kernel 1 or 3, pad = k/2) + bias + activation
 * (0 none, 1 ReLU, 2 exact GELU).  Same conventions as above. */
int ocrvi_test_conv(int device, int dtype, const float* x, const float* weight_host, const float* bias_host,
                    int N, int C, int H, int W, int Co, int ksize, int sh, int sw, int groups, int act, float* out,
                    int iters, float* avg_ms);
/* Stride-1 conv2d (square kernel 1 or 3, pad = k/2) with a residual in the epilogue: out = act(conv(x) + bias + res).  res_mode 1: res
 * is float32 NCHW [N,Co,H,W] (Bottleneck conv3, BasicBlock conv2); res_mode 2: res is [N,Co,H/2,W/2] and is added nearest-2x upsampled,
 * out[.., oh, ow] += res[.., oh/2, ow/2] (the FPN laterals, neck.py:36-38; H and W must be even); res NULL with res_mode 0: no residual.
 * res is converted to NHWC in the compute type exactly as x is.  Same conventions as ocrvi_test_conv. */
int ocrvi_test_conv_res(int device, int dtype, const float* x, const float* weight_host, const float* bias_host, const float* res, int N,
                        int C, int H, int W, int Co, int ksize, int res_mode, int act, float* out, int iters, float* avg_ms);
/* The fused ResNet-50 layer1 chain of the f16x2 detector (csrc/bneck_tail.h) as ONE launch: conv2 3x3 64->64 + ReLU, conv3 1x1 64->256 +
 * identity + ReLU -> y_out, and (no_phase_c = 0) the next block's conv1 1x1 256->64 + ReLU -> t1n_out.  t1: float32 NCHW device [N,64,H,W];
 * identity: [N,256,H,W]; y_out: [N,256,H,W]; t1n_out: [N,64,H,W] (ignored with no_phase_c = 1, as are w1_host / b1_host).  Host weights:
 * w2 [64][64][3][3], w3 [256][64], w1 [64][256]; biases [64] / [256] / [64] or NULL.  Same conventions as ocrvi_test_conv. */
int ocrvi_test_bneck_tail(int device, const float* t1, const float* identity, const float* w2_host, const float* b2_host,
                          const float* w3_host, const float* b3_host, const float* w1_host, const float* b1_host, int N, int H, int W,
                          int no_phase_c, float* y_out, float* t1n_out, int iters, float* avg_ms);
/* The DB head's two deconvolutions (head.py:13-16) as the detector runs them: ConvTranspose2d(64,64,2,2) + folded BN + ReLU of both
 * branches packed as one grouped GEMM (group 0 = binarise, 1 = threshold), ConvTranspose2d(64,1,2,2) in its epilogue.  dc1_w_*: host
 * [64][64][2][2] (c_in, c_out, a, b), dc1_b_*: host [64], dc2_w_*: host [64][1][2][2], dc2_b_*: host [1].
 * groups = 2, binary_only = 0: x float32 NCHW device [N,128,OH,OW] (channels 0..63 are the binarise branch's input, 64..127 the threshold
 * branch's); out = bin_logits, out2 = thresh_logits, float32 device [N,1,4*OH,4*OW].
 * groups = 1, binary_only = 1: the binarise-branch view of the same packed weights, as ocrvi_det_forward_binary launches it; x is
 * [N,64,OH,OW]; out = sigmoid(bin_logits); out2 is not used.  Any other combination, or out2 NULL with binary_only = 0, is OCRVI_EINVAL. */
int ocrvi_test_db_tail(int device, int dtype, const float* x, const float* dc1_w_bin_host, const float* dc1_b_bin_host,
                       const float* dc1_w_thr_host, const float* dc1_b_thr_host, const float* dc2_w_bin_host, const float* dc2_b_bin_host,
                       const float* dc2_w_thr_host, const float* dc2_b_thr_host, int N, int OH, int OW, int groups, int binary_only,
                       float* out, float* out2, int iters, float* avg_ms);
/* Linear / 1x1 convolution as a plain GEMM with the fused epilogue of the hot path: out[M][N] = act(a[M][K] . weight[N][K]^T + bias
 * (+ res)) (res_post = 0) or act(...) + res (res_post = 1); a, res and out are float32 DEVICE buffers (converted to/from `dtype`
 * around the call; the residual is kept in fp32 when out_f32 is set, as the recogniser's residual stream is), weight/bias HOST.  Takes
 * the persistent LDS-DMA ring GEMM whenever the shape is eligible (svtrv2.py:51-61,80-86 Linears; resnet Bottleneck 1x1 convs). */
int ocrvi_test_gemm(int device, int dtype, const float* a, const float* weight_host, const float* bias_host, const float* res, int M,
                    int K, int N, int act, int res_post, int out_f32, float* out, int iters, float* avg_ms);
/* The same call with the output buffer owned by the caller: out_raw is a DEVICE buffer of at least M rows of N output elements (float32
 * when out_f32 is set or `dtype` is OCRVI_F32, else `dtype` elements) that the kernel writes directly (the caller pre-fills it, and any
 * rows past M, and reads the bytes back); only its first M rows are converted to out [M][N] float32 DEVICE. */
int ocrvi_test_gemm_raw(int device, int dtype, const float* a, const float* weight_host, const float* bias_host, const float* res, int M,
                        int K, int N, int act, int res_post, int out_f32, void* out_raw, float* out);
/* Host-only (no GPU): which build of the ring GEMM a plain NHWC convolution of M output pixels, N output channels and GEMM depth K takes
 * on a device of n_cu compute units, from the same function the launcher dispatches on.  amode 0: 1x1 / nn.Linear (K = C_in); amode 1:
 * 3x3, stride 1, pad 1 (K = 9 C_in).  has_res: a residual of the output's shape and element type.  plan = {eligible for the ring GEMM
 * (0 / 1), tile rows BM, tile columns BN, 16-row slices per slice group SPS, fp32-output build (0 / 1), workgroups, fewest row tiles
 * one workgroup walks, most row tiles one workgroup walks}; entries 1..7 describe the ring launch whether or not entry 0 is set. */
int ocrvi_test_ring_plan(int dtype, int amode, int M, int K, int N, int out_f32, int has_res, int n_cu, int32_t plan[8]);
/* ocrvi_test_conv (grouped, strided; square kernel 1 or 3, pad = k/2) with the recogniser's epilogues and the output buffer owned by the
 * caller.  res: NULL, or float32 NCHW DEVICE [N,Co,Ho,Wo], added before the activation (res_post = 0) or after it (res_post = 1); it is
 * kept in fp32 when the output is fp32 (out_f32 set, or `dtype` OCRVI_F32) and cast to `dtype` otherwise.  out_raw: a DEVICE buffer of at
 * least N Ho Wo rows of Co output elements (NHWC; float32 or `dtype` elements) that the kernel writes directly; the caller pre-fills it, and
 * any rows past N Ho Wo, and reads the bytes back.  in_place (needs res and an fp32 output): the residual is copied into out_raw and that
 * one buffer is passed as residual and as output, as the recogniser runs LocalMixing's second convolution on its residual stream.  Only
 * the first N Ho Wo rows are converted to out, float32 NCHW DEVICE [N,Co,Ho,Wo]. */
int ocrvi_test_conv_raw(int device, int dtype, const float* x, const float* weight_host, const float* bias_host, const float* res, int N,
                        int C, int H, int W, int Co, int ksize, int sh, int sw, int groups, int act, int res_post, int out_f32, int in_place,
                        void* out_raw, float* out);
/* Host-only (no GPU): which kernel the 3x3 (pad 1) convolution of ocrvi_test_conv_raw takes on a device of n_cu compute units, from the
 * functions the launcher dispatches on.  has_res: a residual of the output's shape and element type.  plan = {kernel: 0 conv_gemm, 1
 * gconv32, 2 another (conv3_halo, ring GEMM); conv_gemm's tile rows BM and columns BN (0 otherwise); gconv32's output rows per tile th,
 * 16-pixel blocks per tile row nbx, tiles down an image bands_y and across it bands_x (0 otherwise); grid.x; fewest and most tiles one
 * workgroup walks; grid.y = groups; 128-byte K-steps of the packed weights}. */
int ocrvi_test_gconv_plan(int dtype, int N, int C, int H, int W, int Co, int sh, int sw, int groups, int out_f32, int has_res, int n_cu,
                          int32_t plan[12]);
/* The three halo-tile kernels of the f16x2 detector with the output buffers owned by the caller, as ocrvi_test_conv_raw: each *_raw
 * buffer is a DEVICE buffer of at least as many NHWC rows of f16x2 elements (`dtype` elements for the stem) as the output has pixels; the
 * kernel writes it directly, the caller pre-fills it, and any rows past the output, and reads the bytes back; only the output's rows are
 * converted to the float32 NCHW DEVICE tensors.  Each returns OCRVI_EINVAL when the call would not take the kernel named.
 * ocrvi_test_conv3_halo_raw: the dense 3x3 (stride 1, pad 1, bias, act 0 none / 1 ReLU) of ocrvi_test_conv in OCRVI_F16X2 on
 * conv3_halo_kernel: C a multiple of 32, Co a multiple of 4 up to 256, weights packed as (hi, lo) quartets; out_raw [>= N H W][Co].
 * ocrvi_test_bneck_tail_raw: ocrvi_test_bneck_tail into y_raw [>= N H W][256] and t1n_raw [>= N H W][64] (unused with no_phase_c = 1).
 * ocrvi_test_stem_pool_raw: ocrvi_test_stem_pool into out_raw [>= N H/4 W/4][64]; fused != 0 needs stem_pool_eligible. */
int ocrvi_test_conv3_halo_raw(int device, const float* x, const float* weight_host, const float* bias_host, int N, int C, int H, int W, int Co,
                              int act, void* out_raw, float* out);
int ocrvi_test_bneck_tail_raw(int device, const float* t1, const float* identity, const float* w2_host, const float* b2_host,
                              const float* w3_host, const float* b3_host, const float* w1_host, const float* b1_host, int N, int H, int W,
                              int no_phase_c, void* y_raw, void* t1n_raw, float* y_out, float* t1n_out);
int ocrvi_test_stem_pool_raw(int device, int dtype, const float* x, const float* weight_host, const float* bias_host, int N, int H, int W,
                             int fused, void* out_raw, float* out);
/* Host-only (no GPU): the launch of those kernels on a device of n_cu compute units, from the functions their launchers launch on.
 * kind 0: conv3_halo for the C -> Co layer of ocrvi_test_conv3_halo_raw; 1: bneck_tail (either form; C, Co ignored); 2: the fused stem
 * (H, W the image's; C, Co ignored).  plan = {takes the kernel (0 / 1), columns of a column tile NC, column tiles, pixel tiles across an
 * image tiles_x, down it tiles_y (16 x 16 output pixels; the stem: 8 x 7 pooled pixels), workgroups, fewest and most pixel tiles one
 * workgroup walks}. */
int ocrvi_test_halo_plan(int kind, int N, int C, int H, int W, int Co, int n_cu, int32_t plan[8]);
/* Multi-head self-attention on a packed qkv tensor [B, N, 3*heads*32] float32 (layout of
 * qkv.reshape(B,N,3,heads,32), svtrv2.py:80) -> out [B, N, heads*32] float32 (svtrv2.py:82-85). */
/* The detector's stem: conv 7x7 stride 2 pad 3 (3 -> 64 channels) + bias + ReLU + max-pool 3x3 stride 2 pad 1 (torchvision resnet50's
 * conv1 / bn1 / relu / maxpool with BN folded, backbone.py:34).  fused != 0: the one-kernel f16x2 form (dtype must be 3), else the two
 * kernels of the other compute types.  x float32 NCHW device [N,3,H,W] (H, W multiples of 4); weight float32 host [64,3,7,7]; bias float32
 * host [64]; out float32 NCHW device [N,64,H/4,W/4].  Test hook: allocates and synchronises internally. */
int ocrvi_test_stem_pool(int device, int dtype, const float* x, const float* weight_host, const float* bias_host, int N, int H, int W, int fused,
                         float* out, int iters, float* avg_ms);
int ocrvi_test_attention(int device, int dtype, const float* qkv, int B, int N, int heads, float* out, int iters,
                         float* avg_ms);

/* The fused MixingBlock MLP of the 16-bit modes and of OCRVI_F16X2 (svtrv2.py:28-39,100): x [M][D] float32 DEVICE, updated in place to
 * x + fc2(gelu(fc1(LayerNorm(x; ln_g, ln_b)))); with want_xn also xn_out [M][D] float32 DEVICE = LayerNorm(x_new; next_g, next_b) rounded to
 * `dtype` (next_g == NULL: x_new rounded to `dtype`).  Weights and vectors are HOST float32 (fc1 [4D][D], fc2 [D][4D]).  D in {128, 256, 384}. */
int ocrvi_test_mlp(int device, int dtype, float* x, const float* ln_g_host, const float* ln_b_host, const float* w1_host, const float* b1_host,
                   const float* w2_host, const float* b2_host, const float* next_g_host, const float* next_b_host, int want_xn, int M, int D,
                   float* xn_out, int iters, float* avg_ms);
/* The same call with the xn buffer owned by the caller: xn_raw is a DEVICE buffer of at least M rows of D * (element size of `dtype`) bytes that
 * the kernel writes directly (the caller pre-fills it, and any rows past M, and reads the bytes back); only its first M rows are converted to
 * xn_out [M][D] float32 DEVICE (may be NULL).  xn is always produced.  x may likewise be longer than M rows: rows past M are not touched. */
int ocrvi_test_mlp_raw(int device, int dtype, float* x, const float* ln_g_host, const float* ln_b_host, const float* w1_host, const float* b1_host,
                       const float* w2_host, const float* b2_host, const float* next_g_host, const float* next_b_host, int M, int D, void* xn_raw,
                       float* xn_out, int iters, float* avg_ms);
/* lin_x2_kernel (the token-stationary f16x2 Linear of the recogniser's qkv-type layers) on its own: out = a W^T + b in OCRVI_F16X2.
 * a [M][K] float32 DEVICE (cast on the device), weight_host [N][K], bias_host [N] or NULL; K is 256 or 384, N % 32 == 0.  out [M][N] float32
 * DEVICE: the f16x2 result decoded.  out_raw: NULL, or the caller's own DEVICE buffer of at least M rows of N * 4 bytes that the kernel
 * writes directly (rows past M must come back untouched).  max_workgroups > 0 caps the grid, so that a workgroup walks several row tiles
 * at small M.  iters > 0: avg_ms = mean time of `iters` launches. */
int ocrvi_test_lin_x2(int device, const float* a, const float* weight_host, const float* bias_host, int M, int K, int N, int max_workgroups,
                      void* out_raw, float* out, int iters, float* avg_ms);
/* gconv_x2_kernel (LocalMixing's grouped 3x3, stride 1, pad 1, 32 channels per group in and out, OCRVI_F16X2) on its own, arguments as
 * ocrvi_test_conv_raw with Co = C and groups = C / 32.  Two epilogues: out_f32 = 0 and res NULL: act(conv + bias) as f16x2; out_f32 = 1, res
 * and res_post = 1: act(conv + bias) + res in float32 (in_place: the residual is copied into out_raw, which is then residual and output).
 * Anything else, or a shape the kernel does not take, returns OCRVI_EINVAL.  max_workgroups > 0 caps the workgroups per group, so that a
 * workgroup walks several tiles.  With OCRVI_GCONV32=0 the same call runs where the model then runs it, on conv_gemm (A/B timing).
 * iters > 0: avg_ms = mean time of `iters` launches (they repeat the call: do not time an in_place one for its values). */
int ocrvi_test_gconv_x2(int device, const float* x, const float* weight_host, const float* bias_host, const float* res, int N, int C, int H, int W,
                        int act, int res_post, int out_f32, int in_place, int max_workgroups, void* out_raw, float* out, int iters, float* avg_ms);
/* Host-only (no GPU): the tiling of that launch on a device of n_cu compute units.  plan = {rows per tile bh, 16-pixel blocks per tile row
 * nbx, tiles down an image bands_y and across it bands_x, tiles per group, workgroups per group, fewest and most tiles one workgroup walks,
 * groups, dynamic LDS bytes}. */
int ocrvi_test_gconv_x2_plan(int N, int C, int H, int W, int n_cu, int max_workgroups, int32_t plan[10]);
/* Host-only (no GPU): the OCRVI_F16X2 weight format.  src: n fp32 values of one layer (n % 4 == 0) -> dst: n 4-byte elements, per chunk of
 * 4 consecutive elements [hi0 hi1 hi2 hi3 | lo0 lo1 lo2 lo3] (fp16), hi + lo = src * 2^s with one power of two s per layer that puts the
 * largest magnitude into [2^13, 2^14); *wscale = 2^-s.  (What ocrvi_*_create does to every GEMM weight in that mode.) */
int ocrvi_test_pack_f16x2(const float* src, size_t n, void* dst, float* wscale);
/* Host-only (no GPU): the bytes a weight packer hands to its kernel, weights float32 HOST.  kind
 *   0  pack_lin_x2_stream(w0 [N = d0][K = d1])                                          (the stream carries its scale behind the units)
 *   1  pack_mlp_stream(fc1 = w0 [4D][D], fc2 = w1 [D][4D], D = d0, dtype = d1)          (f16x2: likewise)
 *   2  pack_bneck_tail(w3 = w0 [256][64], w1 = the next conv1 [64][256] or NULL): the tail stream; scales = {ws3, ws1}
 *   3  pack_conv of a 3x3 layer w0 [Co = d1][C = d0][3][3] for conv3_halo (f16x2, halo): the quartet form; scales[0] = wscale
 *   4  pack_conv of the same for the deformable convolution's pipelined kernel (f16x2): the quartet form; scales[0] = wscale
 * *size = the byte count; out NULL: nothing else is written, else out [cap >= *size] receives the bytes.  scales: what the kernel's
 * epilogue multiplies by (1.0 where the kind has none). */
int ocrvi_test_pack_stream(int kind, const float* w0, const float* w1, int d0, int d1, void* out, size_t cap, size_t* size, float scales[2]);
/* Host-only (no GPU): the XOR swizzle of rows 0 .. 63 of a [rows][128 B] LDS image, as the packers above and the kernels compute it: the
 * 16-byte position P of row r is kept at P ^ swizzle(r).  swz128: row bits 1 and 3 (bits 0 and 2 of the value); swz_halo: row bits 1 and 2. */
int ocrvi_test_swizzles(int32_t swz128_rows[64], int32_t swz_halo_rows[64]);
/* Host-only (no GPU): the grid of a persistent kernel that walks ntile > 0 tiles on `slots` workgroup slots: at most min(ntile, slots)
 * workgroups, and no more than the longest walk needs. */
int ocrvi_test_persistent_grid(int ntile, int slots, int32_t* grid);

/* The memory-bound kernels of the hot path, one hook each.  Same conventions as above: float32 DEVICE tensors in and out (converted to and
 * from `dtype`, the element type the kernel runs in, around the call), weights and vectors float32 HOST; each hook allocates, binds the
 * f16x2 range flag and synchronises.  No timing arguments. */
/* LayerNorm over the last dim, eps 1e-5 (nn.LayerNorm, svtrv2.py:93,95,446): x [rows][D] -> out [rows][D].  x_f32 / out_f32 != 0: the kernel
 * reads / writes float32 directly (the residual stream), else `dtype` elements.  D % 4 == 0, D <= 1024. */
int ocrvi_test_layernorm(int device, int dtype, const float* x, int x_f32, int out_f32, const float* gamma_host, const float* beta_host,
                         int rows, int D, float* out);
/* FRM vertical cross-attention with the precomputed query (svtrv2.py:236-243), head_dim 32: kv [B*H*W][2D] (token = h*W + w per image, k in
 * columns 0..D-1, v in D..2D-1), vq host [D] -> out [B*W][D].  1 <= H <= 8, D % 32 == 0. */
int ocrvi_test_frm_vertical(int device, int dtype, const float* kv, const float* vq_host, int B, int H, int W, int D, float* out);
/* Adaptive scale fusion (neck.py:57-79): p2 [N,256,H,W], p3 [N,256,H/2,W/2], p4 [N,256,H/4,W/4], p5 [N,256,H/8,W/8] float32 NCHW; w host
 * [4][1024] (the 1x1 attention conv over the concatenation p2 | up(p3) | up(p4) | up(p5)), b host [4] -> out [N,256,H,W].  H, W % 8 == 0. */
int ocrvi_test_asf(int device, int dtype, const float* p2, const float* p3, const float* p4, const float* p5, const float* w_host,
                   const float* b_host, int N, int H, int W, float* out);
/* MaxPool2d(3, stride 2, padding 1) (torchvision resnet stem, backbone.py:34): x [N,C,H,W] -> out [N,C,(H-1)/2+1,(W-1)/2+1].  C % 8 == 0. */
int ocrvi_test_maxpool(int device, int dtype, const float* x, int N, int C, int H, int W, float* out);
/* DB head maps (head.py:28-40): binary = sigmoid(bin_logits), thresh = sigmoid(thresh_logits), thresh_binary = 1 / (1 + exp(-k (binary -
 * thresh))); n float32 elements per map (n % 4 == 0, 16-byte aligned).  thresh and thresh_binary may be NULL (then not written). */
int ocrvi_test_db_maps(int device, const float* bin_logits, const float* thresh_logits, float k, float* binary, float* thresh,
                       float* thresh_binary, size_t n);
/* The recogniser's decode head (svtrv2.py:536,555): logits [B*T][ld] (row = b*T + t, columns C..ld-1 are never read) -> log_softmax over the
 * C classes into log_probs [T][B][C] and its per-step argmax into argmax_ids [B][T] (first index wins ties; 0 for a row whose log-probs
 * are NaN, as ocrvi_ctc_greedy gives).  Either output may be NULL.  C <= 1024, ld >= C. */
int ocrvi_test_ctc_logsoftmax(int device, const float* logits, int ld, int B, int T, int C, float* log_probs, int32_t* argmax_ids);
/* The same head as ocrvi_rec_forward_conf launches it: also best_lp [B][T], the float32 log_probs[t][b][argmax_ids[b][t]] bit for bit (the
 * NaN of entry 0 for a NaN row).  Any output may be NULL. */
int ocrvi_test_ctc_logsoftmax_conf(int device, const float* logits, int ld, int B, int T, int C, float* log_probs, int32_t* argmax_ids,
                                   float* best_lp);

/* ------------------------------------------------------------------------------------------------
 * Document finder: the corners that four-point rectification takes, found from the page (find_document_contour_dl,
 * src/preprocess/scanner.py:78-132).  The reference gets its mask from the rembg U-2-Net, whose weights are a download and stay out;
 * what is built is (A) its mask-to-corners half, scanner.py:104-132, for any mask the caller has (rembg's alpha included), and (B) a mask of
 * the library's own, computed on the device from the page's luminance.  (B) separates a document from its background by brightness only:
 * a white receipt on a white table gives the frame, a rectangle or nothing.  cv2 is absent from the build container: parity with cv2
 * (findContours' order, boxPoints' rounding) is UNPINNED; tests/docfind_ref.py restates both halves and must agree to the last bit.
 * ------------------------------------------------------------------------------------------------ */
/* (A) Host only, needs no GPU.  mask: uint8 [h] rows of w pixels, `stride` bytes apart (sides 1 .. 16384); quad int32 [4][2] (x, y) in mask
 * coordinates; *found = 0 none (quad zeroed), 1 a four-point polygon, 2 the rectangle fallback.
 *   foreground  mask != 0, as cv2.findContours sees it
 *   contours    RETR_EXTERNAL, CHAIN_APPROX_SIMPLE: the outer borders (Suzuki-Abe border following, as ocrvi_db_postprocess) of the
 *               8-connected components that no other component encloses; hole borders and components inside a hole are dropped.  Their
 *               order is that of the RETR_LIST scan, last found first, restricted to these.
 *   candidates  sorted by contourArea (shoelace) in descending order, stable; the first five
 *   polygon     the first candidate whose approxPolyDP(cnt, 0.02 * arcLength(cnt, True), True) has exactly four points, in its order
 *   fallback    otherwise the minimum-area rectangle of the largest contour as ocrvi_min_area_quads defines it (a degenerate hull gives the
 *               bounding-box corners), each coordinate truncated toward zero (np.int32(cv2.boxPoints(...))) */
int ocrvi_document_contour(const uint8_t* mask, int h, int w, int64_t stride, int32_t* quad /*[4][2]*/, int32_t* found);
/* The same on the bit mask (B) produces: bit x & 31 of word y * ((w + 31) / 32) + (x >> 5). */
int ocrvi_document_contour_bits(const uint32_t* bits, int h, int w, int32_t* quad /*[4][2]*/, int32_t* found);

/* (B) The library's own mask.  Integer arithmetic except where stated; work_h (8 .. 512) is the working image's height, 500 in the reference.
 *   size      ratio = H / (double)work_h;  ww = int(W / ratio) in IEEE double (scanner.py:85-86);  8 <= ww <= 8192, page sides <= 16384
 *   grey      working pixel (i, j) covers source rows [i H / work_h, max(that + 1, (i + 1) H / work_h)) (floor divisions) and columns
 *             likewise with W and ww; luma = (77 R + 150 G + 29 B + 128) >> 8 per source pixel; G = (sum + n / 2) / n over the box's n pixels
 *   smooth    [1 4 6 4 1] along x and along y, replicate border; S = (sum + 128) >> 8
 *   histogram 256 bins of S
 *   Otsu      N = sum h, mT = sum v h[v]; for t = 0 .. 254: w0 = sum_{v <= t} h[v], m0 = sum_{v <= t} v h[v], w1 = N - w0; t is skipped when
 *             w0 = 0 or w1 = 0; d = mT w0 - m0 N exactly (|d| < 2^53); score = (double(d) * double(d)) / (double(w0) * double(w1)) in IEEE
 *             double, in this order, no fused multiply-add; the smallest t of maximal score.  A single non-empty bin: no threshold (t = -1),
 *             the mask is all zero.
 *   polarity  B = S > t.  OCRVI_DOC_AUTO: when more than half of the ring's pixels (the outermost rows and columns, each once) are set,
 *             B is inverted -- the frame is background; a tie keeps B.  OCRVI_DOC_BRIGHT keeps B, OCRVI_DOC_DARK inverts it.
 *   opening   5 x 5 square erosion, then 5 x 5 dilation; pixels outside the image are background in both
 *   output    one bit per working pixel, bit x & 31 of word y * ((ww + 31) / 32) + (x >> 5); padding bits are zero
 * All entries below are enqueue-only on `stream` (no allocation, no synchronisation); every pointer is DEVICE memory unless stated. */
#define OCRVI_DOC_AUTO 0
#define OCRVI_DOC_BRIGHT 1
#define OCRVI_DOC_DARK 2
/* Host only: *ww and *ratio of an h x w page by the size rule; OCRVI_EINVAL outside the bounds above. */
int ocrvi_doc_working_size(int h, int w, int work_h, int32_t* ww, double* ratio);
/* Host only: the workspace of ocrvi_doc_mask_pages for n pages (1 .. 65535) whose working widths are at most ww_cap, and the uint32 words
 * of one page's slot in `masks`, work_h * ((ww_cap + 31) / 32). */
int ocrvi_doc_mask_sizes(int n, int work_h, int ww_cap, size_t* workspace_bytes, size_t* mask_words);
/* The whole of (B) for n pages of their own sizes: `pages` is a page table (OCRVI_PAGE_ENTRY), read when the kernels run.  Page i's mask
 * starts at masks + i * mask_words and is laid out by ITS OWN ww.  An invalid entry, a side above 16384 or a working width outside
 * [8, ww_cap] leaves the page's slot all zero and touches nothing else.  workspace: 16-byte aligned. */
int ocrvi_doc_mask_pages(int device, const int64_t* pages, int n, int work_h, int ww_cap, int polarity, uint32_t* masks, void* workspace,
                         size_t workspace_bytes, void* stream);
/* The stages one by one.  src uint8 HWC [h,w,3] -> dst uint8 [work_h][ww] (grey); uint8 [work_h][ww] -> the same (smooth, dst != src); ->
 * hist int32 [256] (zeroed by the call); smooth + hist -> thr int32 [4] = (t, inverted 0 / 1, 0, 0); smooth + thr -> bits. */
int ocrvi_doc_grey_u8(int device, const uint8_t* src, int h, int w, int work_h, uint8_t* dst, void* stream);
int ocrvi_doc_smooth_u8(int device, const uint8_t* src, int work_h, int ww, uint8_t* dst, void* stream);
int ocrvi_doc_histogram(int device, const uint8_t* src, int work_h, int ww, int32_t* hist, void* stream);
int ocrvi_doc_otsu(int device, const uint8_t* smooth, const int32_t* hist, int work_h, int ww, int polarity, int32_t* thr, void* stream);
int ocrvi_doc_mask_bits(int device, const uint8_t* smooth, int work_h, int ww, const int32_t* thr, uint32_t* bits, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Skew estimate: by how much a page is rotated, from the page alone, and the corners that straighten it.  The reference has no such
 * step; it sits where `--preprocess` sits, for pages whose border the document finder cannot see (a flatbed or feeder scan fills the
 * frame).  A projection-profile search: text lines binned along the right slope give a profile of sharp peaks, whose sum of squares is
 * maximal.  Integer arithmetic throughout; tests/skew_ref.py restates every stage and must agree exactly.  work_h (8 .. 512), ww, ratio
 * and the bounds are those of ocrvi_doc_working_size; G is the document finder's `grey` stage, unchanged.
 *   edges    d = |G[i][min(j+1, ww-1)] - G[i][max(j-1, 0)]|;  E[i][j] = d >= OCRVI_SKEW_FLOOR ? d : 0  (the horizontal central difference,
 *            replicated border: horizontal rules contribute nothing, vertical rules the same to every row)
 *   offset   for the slope index k in -OCRVI_SKEW_K .. OCRVI_SKEW_K and column j:  o(j, k) = ((j - (ww >> 1)) * k + 256) >> OCRVI_SKEW_SHIFT,
 *            an arithmetic shift (a floor; the product may be negative)
 *   profile  P_k[r] = the sum of E[i][j] over all (i, j) with i - o(j, k) == r, for every integer r  (an int32: 255 * 8192 < 2^31)
 *   score    S_k = the sum over r of P_k[r]^2, an exact uint64 (< 2^54), independent of the order;  scores[k + OCRVI_SKEW_K] = S_k
 *   pick     (host) the k of maximal S_k; among equals the smallest |k|; of -k and +k, +k.  angle_deg = atan(k / 512.0) * 180 / pi and
 *            gain = double(S_best) / double(S_0) in double; when S_0 == 0 the gain is 1.0 if S_best == 0 and +inf otherwise.  A constant
 *            page gives k = 0.  A text line of image slope tan(theta), y pointing down, is picked at k ~ 512 tan(theta): the range is
 *            +-14.04 degrees in steps of 0.112 degrees.
 *   quad     (host, double, no fused multiply-add, in this order)  t = k / 512.0, c = 1 / sqrt(1 + t t), s = t c;  centre (cx, cy) =
 *            ((w-1) / 2, (h-1) / 2);  for the page's corners (0,0) (w,0) (w,h) (0,h):  dx = x - cx, dy = y - cy, a = dx c + dy s,
 *            b = dy c - dx s;  the quad is (cx + a c - b s, cy + a s + b c) for (a, b) = (amin,bmin) (amax,bmin) (amax,bmax) (amin,bmax):
 *            the upright rectangle of the deskewed frame that encloses the whole page, so no content is lost and the wedges outside the
 *            page are the warp's 0.  ocrvi_four_point_transform orders these corners as given and decides the output size; k = 0 gives
 *            the page's own corners and its own size.
 * The device entries are enqueue-only on `stream` (no allocation, no synchronisation); pointers are DEVICE memory unless stated. */
#define OCRVI_SKEW_K 128
#define OCRVI_SKEW_SHIFT 9
#define OCRVI_SKEW_FLOOR 8
#define OCRVI_SKEW_ANGLES 257
/* Host only: the workspace of ocrvi_skew_scores_pages for n pages (1 .. 65535) whose working widths are at most ww_cap. */
int ocrvi_skew_sizes(int n, int work_h, int ww_cap, size_t* workspace_bytes);
/* grey -> edges -> scores for n pages of their own sizes: `pages` is a page table (OCRVI_PAGE_ENTRY), read when the kernels run; page i's
 * scores are scores[i][0 .. 256].  An invalid entry, a side above 16384 or a working width outside [8, ww_cap] leaves the page's 257 scores
 * zero and touches nothing else.  workspace: 16-byte aligned; scores: 8-byte aligned. */
int ocrvi_skew_scores_pages(int device, const int64_t* pages, int n, int work_h, int ww_cap, uint64_t* scores /*[n][257]*/, void* workspace,
                            size_t workspace_bytes, void* stream);
/* The stages one by one, on row-major arrays: grey uint8 [work_h][ww] -> edges (edges != grey); edges of ANY values -> scores [257]. */
int ocrvi_skew_edges_u8(int device, const uint8_t* grey, int work_h, int ww, uint8_t* edges /*[work_h][ww]*/, void* stream);
int ocrvi_skew_scores(int device, const uint8_t* edges /*[work_h][ww]*/, int work_h, int ww, uint64_t* scores /*[257]*/, void* stream);
/* Host only: pick and quad as defined above.  scores: HOST [257];  quad: float64 [4][2] of (x, y);  1 <= h, w <= 16384, |k| <= 128. */
int ocrvi_skew_pick(const uint64_t* scores, int32_t* k, double* angle_deg, double* gain);
int ocrvi_skew_quad(int h, int w, int k, double* quad /*[4][2]*/);

/* Per-launch HIP-event profiler (process-global, off by default).  While enabled every MFMA / bandwidth kernel launch
 * of the graphs above is bracketed by two events recorded on its launch stream.  ocrvi_prof_report synchronises those
 * events and writes a JSON object {tag: {launches, ms, flops, bytes}} (algorithmic FLOPs / bytes per tag) into buf. */
int ocrvi_prof_enable(int on);
int ocrvi_prof_reset(void);
int ocrvi_prof_report(char* buf, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* OCRVI_H */
