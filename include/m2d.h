/* m2d.h -- C ABI of the MI355X (gfx950) Market2Dish scoring engine (libm2d.so).
 *
 * The reference (WenjieWWJ/FoodRec) has no FFI: its boundary is a Python class plus TF1 session
 * fetches.  Each entry point below names the reference interface it stands in for (paths relative
 * to the reference root, Code/Recommender/...).  The Python layer (foodrec_amd/) is the only
 * caller; it registers these as torch.library custom ops (foodrec_amd/ops.py).
 *
 * Conventions
 *   - every function returns an int status: M2D_OK (0) or a negative M2D_ERR_* code; nothing throws;
 *   - data pointers are DEVICE pointers (HBM) unless a parameter says "host"; the caller owns every
 *     buffer; the engine owns only what it allocates itself (tables passed with M2D_TABLES_HOST);
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); kernels are enqueued and
 *     the call returns without synchronising.  Id errors found by a kernel are latched on the
 *     device and reported by m2d_check(), which does synchronise;
 *     WHERE A CALL DOES WAIT.  Always, by design: m2d_check and m2d_train_begin wait for `stream`; m2d_score_pairs_host waits for
 *     its own work on `stream`; m2d_cookable_dishes waits for `stream` once, for the count (and with it whatever calls it first:
 *     the Python layer's topk_market); the setters (m2d_set_*) work on the NULL stream and wait for it, which orders nothing for a
 *     stream created non-blocking: call them with no work of the engine in flight; m2d_clear_*, m2d_train_end, m2d_train_steps and
 *     the read-only diagnostics of m2d_get_option wait for the whole device.
 *     Once, and then not again until the cause recurs: the first call that runs on m2d_topk_users' retrieval plan (that call and
 *     the calls defined through it) after m2d_create, a setter, m2d_train_step or m2d_tables_updated waits for `stream` once it
 *     has queued the build of the pattern-grouped dish rows (it reads the tile count, the "masks are 0/1" flag and the "a table
 *     value is not finite" word); the first such call after the table scan or after m2d_write_memory waits for the whole device
 *     before it reads that word again; a call that has to grow one of the engine's buffers (the first call of a size;
 *     m2d_train_step with a larger batch than any before) frees the old block, which waits for the device.  A call that finds its
 *     tables built and its buffers large enough returns without waiting: the pair-scoring calls from their second call of a size
 *     on, m2d_topk_markets and the others that say "never synchronises" below.
 *     Wherever a call waits, it waits for `stream` BEFORE it reads the device on the host, and everything it queues -- a lazy build
 *     included -- it queues on `stream`: inputs that an earlier copy on `stream` is still writing when the call is made are read as
 *     that copy leaves them.  tests/test_gpu_stream_order.py holds the entry points that take device buffers to this on a
 *     non-default stream, as an engine's first call and again on the engine so warmed: the inputs are overwritten by copies queued
 *     behind a 0.1 s blocker, the call is made while the blocker runs, and the result must be the one a second engine returns for
 *     the late inputs on the null stream.  (m2d_write_memory and m2d_train_step: as a first call only);
 *   - an engine is not thread-safe; distinct engines / streams are independent;
 *   - all arithmetic is float32; ids are int32 (Model_Recommender.py:26-32).
 *
 * Setters (m2d_set_dish_categories, m2d_set_ingredients, m2d_set_recipes, m2d_set_mlp_head, m2d_train_begin) fail in one of two ways:
 *   - refused BEFORE anything is replaced -- whatever the arguments alone decide: a null pointer, a size, bad `table_flags`, a
 *     BORROWED array (M2D_TABLES_DEVICE) that must be 16-byte aligned and is not (the dish masks; W1 and W2 of the head), and, where
 *     the setter reads the id-error latch first, an id error still latched from an earlier launch, returned under its own code.
 *     The previous table / head / ingredients / recipes / training state stays set and served, its borrowed arrays still borrowed;
 *   - failed AFTER replacement has begun -- a HIP error, a copy of the engine's own that is not aligned, a malformed CSR, a bad id:
 *     the feature is left UNSET, exactly as the matching m2d_clear_* / m2d_train_end leaves it, and the call returns its own code and
 *     text.  The engine never keeps a pointer from a call it refused, and never serves a half-set feature.
 * What a setter builds lazily from its tables later follows the same rule: a build that fails leaves nothing behind that a later
 * call would take for built.
 */
#ifndef M2D_H_
#define M2D_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct m2d_engine m2d_engine;

#define M2D_OK 0
#define M2D_ERR_INVALID_ARG (-1)    /* null pointer, non-positive size, k out of range ...          */
#define M2D_ERR_HIP (-2)            /* a HIP runtime call failed; text in m2d_last_error()           */
#define M2D_ERR_BAD_USER_ID (-3)    /* a user id outside [user_base, user_base + U)                  */
#define M2D_ERR_BAD_ITEM_ID (-4)    /* a dish id outside [0, I)                                      */
#define M2D_ERR_NOT_CONFIGURED (-5) /* call needs m2d_set_dish_categories / m2d_set_* first          */
#define M2D_ERR_UNSUPPORTED (-6)    /* shape outside what the kernels cover (message says which)     */
#define M2D_ERR_NO_DEVICE (-7)      /* no HIP device visible: there is no CPU fallback, by design    */
#define M2D_ERR_BAD_INGREDIENT (-8) /* extension: ingredient id outside [0, R) or a malformed CSR     */
#define M2D_ERR_KERNEL_TIMEOUT (-9) /* m2d_topk_users: a wave gave up waiting for its workgroup (about 1 s); that call's
                                       lists are INVALID.  Latched on the device, reported by m2d_check */

#define M2D_TABLES_HOST 0   /* table pointers are host memory: copied to HBM once, engine-owned      */
#define M2D_TABLES_DEVICE 1 /* table pointers are device memory: borrowed, caller keeps them alive   */

/* ABI version: bumped on any signature change. */
int m2d_abi_version(void);

/* Model build.  Replaces Model.__init__ + instantiate_weights (Model_Recommender.py:5-37, :43-54):
 *   pm [U, C+1, E]  Personal_Memory  (row 0 high-level, rows 1..C low-level per category)
 *   re [I, E]       Recipe_Embedding
 *   ce [C, E]       Category_Embedding
 *   coef            high_level_score_coefficient, held as float32; (1 - coef) is taken in float32
 *                   (Model_Recommender.py:17, :96)
 * General_Memory is not an argument: the forward never reads it (Model_Recommender.py:56-97). */
int m2d_create(const float *pm, const float *re, const float *ce, int64_t U, int64_t I, int32_t C,
               int32_t E, float coef, int device, int table_flags, m2d_engine **out);
int m2d_destroy(m2d_engine *h);

/* Text of the last failure on this engine (or of the last failed m2d_create when h == NULL). */
const char *m2d_last_error(const m2d_engine *h);

/* User-axis sharding (no reference counterpart): this engine holds users
 * [user_base, user_base + U); ids in every call stay GLOBAL. */
int m2d_set_user_base(m2d_engine *h, int64_t user_base);

/* Resident per-dish category masks [I, C] -- the device-side form of dish_to_category.json
 * (Train_recommender.py:132, evaluate.py:43,50).  Needed by the *_bydish / rank / topk calls.  The table is read 16 bytes at a
 * time: a borrowed one must be 16-byte aligned.  Failures: "Setters" above. */
int m2d_set_dish_categories(m2d_engine *h, const float *cats, int table_flags);

/* Predict.  Replaces sess.run([model.logits], feed_dict) (evaluate.py:55-59) = Model.inference
 * (Model_Recommender.py:56-97) for B pairs:
 *   users i32[B], items i32[B], cats f32[B, C] (the [B, C, 1] placeholder flattened; any float
 *   weight is accepted, a row summing to 0 yields NaN as 0/0 does at :79/:92), out f32[B]. */
int m2d_score_pairs(m2d_engine *h, const int32_t *users, const int32_t *items, const float *cats,
                    int64_t B, float *out, void *stream);

/* m2d_score_pairs for HOST buffers -- what the reference's call site actually hands over (lists / numpy, 51 pairs
 * per call, evaluate.py:39-59).  users, items, cats and out are host pointers; the call puts them in one pinned
 * block, WAITS for the work it enqueued on `stream` and returns the scores in `out`.  Up to 65 536 pairs the kernel
 * reads and writes that block over the host link and the call spins on a completion word behind the scores before it
 * falls back to a stream wait; larger feeds (or option "host_zero_copy" = 0) take one copy in and one copy out
 * (1 = pinned block without the spin); feeds of more than 262 144 pairs go in chunks of that size through two
 * pinned blocks, the host's copy of one chunk overlapping the transfer and kernel of the one before (0.66 -> 1.0 G
 * pairs/s at 4 M pairs).  Same kernels, same bits either way.  An out-of-range
 * id is returned directly as M2D_ERR_BAD_USER_ID / M2D_ERR_BAD_ITEM_ID (text in m2d_last_error, position counted in
 * the whole feed), `out` untouched -- or, for a chunked feed, holding the scores of the chunks before the offending one.
 * This is the latency path; its rate includes PCIe and is never what bench.py reports as `value`. */
int m2d_score_pairs_host(m2d_engine *h, const int32_t *users, const int32_t *items, const float *cats,
                         int64_t B, float *out, void *stream);

/* Same, with cats looked up from the resident dish table: cats[b] = dish_categories[items[b]]. */
int m2d_score_pairs_bydish(m2d_engine *h, const int32_t *users, const int32_t *items, int64_t B,
                           float *out, void *stream);

/* Evaluator inner step.  Replaces eval_one_rating's scoring + ranking (evaluate.py:35-63) for
 * nseg users in ONE launch: segment s scores users[s] against items[s*L .. s*L + lens[s]) and
 * returns the first k of heapq.nlargest order -- a repeated item keeps its first position and its
 * last score (dict collapse, :60-61), ties go to the earlier position (:63).
 *   lens may be NULL (every segment has L candidates); 1 <= L <= 1024; 1 <= k <= 64
 *   out_items i32[nseg, k] (-1 past the number of distinct candidates), out_scores f32[nseg, k],
 *   out_flags i32[nseg]: bit 0 set when a candidate score is NaN -- the caller must then rank that
 *   segment on the host, where the reference's NaN behaviour can be reproduced exactly. */
int m2d_rank_candidates(m2d_engine *h, const int32_t *users, const int32_t *items, const int32_t *lens,
                        int64_t nseg, int32_t L, int32_t k, float *out_scores, int32_t *out_items,
                        int32_t *out_flags, void *stream);

/* Full-catalogue retrieval (build-defined generalisation of evaluate.py:39-63 to every dish; BASELINE
 * config 5): for each of nU users the k best dishes over all I, descending score, ties to the lower
 * dish id, NaN scores last (after every -inf score).  out_scores f32[nU, k], out_ids i32[nU, k].  1 <= k <= 64.
 * Scores agree with m2d_score_pairs_bydish within the 1e-4 bar, not bit for bit (factored form; see the
 * "topk_bf16x3" option below).
 * While a table value is inf / NaN (the engine's "not finite" word: Personal_Memory, Recipe_Embedding, Category_Embedding; +-inf
 * in H[d] of the ingredient table) every call runs m2d_topk_literal instead, whatever the options: the formula as written, one
 * block per user, untuned.  Its lists are the graph's -- +inf first, -inf after every finite score, NaN last, each in id order --
 * and a listed score is m2d_score_pairs_bydish's under "variant" = 9 bit for bit.
 * Kernels: 0/1 masks, C = 4, k <= 16 and E a multiple of 4 up to 256 run the pattern-grouped MFMA kernels (E = 64 / 128
 * on split bf16 by default; other sizes, e.g. the reference's embed_size 200, exact f32 on dish rows zero-padded to
 * 32 / 64 / 128 / 256 floats); other masks or k run the dense MFMA kernel where (C + 1) E / 8 is 20, 40 or 80, and a
 * one-block-per-user kernel otherwise.
 * With the ingredient table set (m2d_set_ingredients) the high-level term uses H[d]; E = 32 / 64 stay on the
 * pattern-grouped split-bf16 kernel (rows [H[d] | RE[d]]), other shapes use the dense kernel.
 * Tie rule: bit-equal scores resolve to the lower dish id, whatever kernel runs -- heapq.nlargest's rule
 * (evaluate.py:63).  The pattern-grouped kernels scan the dishes grouped by mask pattern and, inside a pattern, by
 * descending row norm; they notice when a tie decides what a list holds (a score equal to a list's last entry falls off
 * or is refused), and such users -- an all-zero Personal_Memory block, a user vector that scores whole groups
 * identically -- are re-ranked over the catalogue in id order with the formula in plain f32 (their scores are then
 * exact-f32 even under "topk_bf16x3" = 1).  Option "topk_grouped" = 0 selects the dense kernel (about 5x the matrix
 * work), which scans in id order.
 * coef = 1 (Train_recommender.py:61-62; `1 - coef` is then an exact float32 zero, Model_Recommender.py:96): every dish of a
 * mask pattern scores alpha_P[u], so the pattern-grouped path reads each list off the patterns' lowest dish ids, best
 * alpha_P first (m2d_topk_high_level_only: no scan, no repair; what heapq.nlargest returns for whole groups of equal scores). */
int m2d_topk_users(m2d_engine *h, const int32_t *users, int64_t nU, int32_t k, float *out_scores,
                   int32_t *out_ids, void *stream);

/* Full-catalogue rank (build-defined; the full-ranking protocol of leave-one-out evaluation).  A query is (user u, held-out dish p),
 * X its optional set of excluded dish ids:
 *     rank = #{ d in [0, I), d not in X, d != p : d precedes p }
 * in m2d_topk_users' order (score descending, NaN scores last, equal scores -- NaN included -- to the lower dish id).  The score is the
 * plain-f32 arithmetic m2d_topk_users finishes near-tied lists in (alpha_P from the retrieval plan's <U_high, CE_c>, a float4 column per
 * lane of 16 in fmaf chains, the 16-lane rotation sum, alpha_P + b low / n_P; an empty mask scores NaN), so wherever retrieval lists are
 * index-exact (default options: E = 32 / 64 with k <= 16, E = 128 with k <= 10) rank(u, ids[u][j]) == j for every listed dish.
 * An id of X equal to p is ignored; repeated ids count once.
 * For n queries (users[i], items[i]): out_rank i32[n] as defined above; out_scores f32[n] (may be NULL) receives the
 * held-out dish's score in the ranking arithmetic.  excl_off i64[n + 1] (NULL = no exclusions) and excl_ids i32[excl_off[n]]
 * are device memory; ids ascending within each segment.
 * Needs the dish masks (M2D_ERR_NOT_CONFIGURED); C = 4, 0/1 masks, finite tables, E a multiple of 4 up to 256, no ingredient table
 * and no MLP head -- anything else is M2D_ERR_UNSUPPORTED, the message naming the condition.  Bad user / held-out / excluded ids are
 * latched as M2D_ERR_BAD_USER_ID / M2D_ERR_BAD_ITEM_ID and a segment that is not ascending as M2D_ERR_INVALID_ARG, reported by
 * m2d_check with their positions (query index; for excluded ids the index into excl_ids).  Diagnostics: "rank_tiles_scanned",
 * "rank_resolved" (m2d_get_option).  The m2d_topk_users diagnostics are left as they were. */
int m2d_catalogue_rank(m2d_engine *h, const int32_t *users, const int32_t *items, int64_t n,
                       const int64_t *excl_off, const int32_t *excl_ids,
                       int32_t *out_rank, float *out_scores, void *stream);

/* Full-catalogue retrieval without each user's excluded dishes (build-defined; the serving half of the full-ranking protocol).  For
 * user i, X_i = excl_ids[excl_off[i] .. excl_off[i + 1]):  out_ids i32[nU, k] / out_scores f32[nU, k] receive the first k dishes of
 * the ranking over { d in [0, I) : d not in X_i } in m2d_topk_users' order (score descending, NaN scores last, equal scores -- NaN
 * included -- to the lower dish id).  Ids are decided and scores written in m2d_catalogue_rank's arithmetic, bit for bit that call's
 * out_scores, so for the same user and X:  m2d_catalogue_rank(u, out_ids[u][j], X) == j  for every listed dish, whatever the options
 * and the launch shape.  When fewer than k dishes remain the row ends in id -1 with a NaN score.
 * excl_off i64[nU + 1] (NULL = no exclusions) and excl_ids are device memory, ids ascending within each segment, repeated ids count
 * once (m2d_catalogue_rank's conventions).  1 <= k <= 16; k > I is M2D_ERR_INVALID_ARG as in m2d_topk_users.
 * Two tiers, both exact.  Where m2d_topk_users' lists are index-exact (default retrieval options, E = 32 / 64 with K1 = 16, E = 128 with
 * K1 = 10, k <= K1) the unfiltered top K1 is retrieved into engine scratch and filtered: it holds every dish that can precede its own
 * last entry, so k survivors are the filtered top k.  Users with fewer survivors -- and every user for other E, larger k or
 * non-default retrieval options -- take an exact scan with exclusions over the patterns that can reach their top k (m2d_catalogue_rank's
 * tables, bounds and arithmetic; csrc/m2d_catalogue_excl.hip).  The call allocates nothing after its first launch of a size and
 * never synchronises.
 * Needs what m2d_catalogue_rank needs: dish masks (M2D_ERR_NOT_CONFIGURED); C = 4, 0/1 masks, finite tables, E a multiple of 4 up to
 * 256, no ingredient table, no MLP head (M2D_ERR_UNSUPPORTED, the message naming the condition).  A bad user id or excluded id is
 * latched as M2D_ERR_BAD_USER_ID / M2D_ERR_BAD_ITEM_ID, a segment (or offset) that is not ascending as M2D_ERR_INVALID_ARG; m2d_check
 * reports them with the user index, or the index into excl_ids / excl_off.  The rows of a call with a latched error are unspecified.
 * m2d_set_user_base is honoured (ids stay global).  Diagnostics: "topk_excl_short", "topk_excl_tiles_scanned"; A/B: "topk_excl_tier".
 * The m2d_catalogue_rank diagnostics are left as they were; the m2d_topk_users diagnostics ("topk_*" below) afterwards describe
 * the call's internal retrieval of K1 entries when the first tier ran, and are left as they were when it did not. */
int m2d_topk_users_excluding(m2d_engine *h, const int32_t *users, int64_t nU, int32_t k,
                             const int64_t *excl_off, const int32_t *excl_ids,
                             float *out_scores, int32_t *out_ids, void *stream);

/* Memory write (training side).  Replaces Model.Write_Memory
 * (Model_Recommender.py:106-220) -- the `personal` / `general` fetches of Train_recommender.py:180-199 --
 * with an O(B (C+1) E) atomic scatter-add in place of the reference's dense one-hot matmuls:
 *     PM[u_b] += v_b + alpha * g_b ;   GM[l] += sum_b y_bl v_b          (v_b, g_b: see csrc/m2d_write.hip)
 *   users/items i32[B], cats f32[B, C], write_sign f32[B] (the [B, 1] placeholder flattened),
 *   labels f32[B, L] (user_one_hot_label), general_memory f32[L, C+1, E] (device, updated in place).
 * Personal_Memory is updated IN PLACE in the buffer given to m2d_create, which must therefore be
 * writable device memory (M2D_TABLES_DEVICE) or engine-owned (M2D_TABLES_HOST).
 * `which` selects the assigns that run, as the fetch list does in the reference graph: `personal` depends on the two
 * chained Personal_Memory assigns only (:167, :198), `general` on the General_Memory assign only (:215) -- the
 * driver's ordinary batch fetches `general` alone (Train_recommender.py:195-199), so it never writes Personal_Memory.
 *   M2D_WRITE_PERSONAL  PM[u_b] += v_b + alpha * g_b      (g_b reads General_Memory as it stands before this call)
 *   M2D_WRITE_GENERAL   GM[l]   += sum_b y_bl v_b
 * out_sums (device f64[2], may be NULL) receives sum(PM) in [0] when M2D_WRITE_PERSONAL is set and sum(GM) in [1]
 * when M2D_WRITE_GENERAL is set, after the write (the reference returns their means); the other entry is 0. */
#define M2D_WRITE_PERSONAL 1
#define M2D_WRITE_GENERAL 2
int m2d_write_memory(m2d_engine *h, const int32_t *users, const int32_t *items, const float *cats,
                     const float *write_sign, const float *labels, int64_t B, int32_t L, float *general_memory,
                     float beta_1, float beta_2, float alpha, int32_t which, double *out_sums, void *stream);

/* Training step.  Replaces Model.loss + Model.train (Model_Recommender.py:99-104,
 * :223-241) as the driver runs them: sess.run([model.loss_value, model.learning_rate, ..., model.train_op], feed_dict)
 * (Train_recommender.py:180-199).  All three tables given to m2d_create are updated IN PLACE and must be writable
 * device memory (M2D_TABLES_DEVICE) or engine-owned; General_Memory gets no gradient and is not involved.
 *   m2d_train_begin  `learner` as the reference's --learner flag (:228-235: adagrad / rmsprop / adam, anything else
 *                    is gradient descent), `lr` = args.lr (the decayed rate equals it for ever: apply_gradients is
 *                    called without global_step, :240), `clip_norm` = 5.0 in the reference (:237).  Allocates the
 *                    optimizer slots (TF 1.x initial values) and scratch; calling it again resets the optimizer.
 *   m2d_train_step   users/items i32[B], cats f32[B, C], labels f32[B].  apply = 1: loss, gradients, global-norm
 *                    clip and the update; apply = 0: loss and gradient norm only (the loss_value fetch alone).
 *                    out (device f32[4], may be NULL) receives {loss, global gradient norm, clip scale, lr}.
 *                    An out-of-range id blocks the whole update (TF raises from the gather before any assign): the
 *                    tables, the slots, the step count and Adam's beta powers all stay as they were.  The id error
 *                    stays latched until m2d_check reports it, and while it is latched every later step is blocked
 *                    too -- call m2d_check after a step whose ids are not known to be valid.
 *   m2d_train_slot   copies optimizer slot `slot` of table 0 = Personal_Memory, 1 = Recipe_Embedding,
 *                    2 = Category_Embedding (adam: m, v; adagrad: accumulator; rmsprop: rms, momentum) into `buf`
 *                    (restore = 0) or from it (restore = 1); `buf` is device memory shaped like the table.  For
 *                    checkpoint / resume (the reference's tf.train.Saver covers the slots too).
 *                    M2D_ERR_INVALID_ARG when the learner has no such slot.
 * The update rules restate TF 1.x's published behaviour (oracle/train_oracle.py); parity is unpinned. */
#define M2D_LEARNER_SGD 0
#define M2D_LEARNER_ADAGRAD 1
#define M2D_LEARNER_RMSPROP 2
#define M2D_LEARNER_ADAM 3
int m2d_train_begin(m2d_engine *h, int32_t learner, float lr, float clip_norm, void *stream);
int m2d_train_step(m2d_engine *h, const int32_t *users, const int32_t *items, const float *cats, const float *labels,
                   int64_t B, int32_t apply, float *out, void *stream);
int m2d_train_slot(m2d_engine *h, int32_t table, int32_t slot, float *buf, int32_t restore, void *stream);
/* Tell the engine that borrowed table memory (M2D_TABLES_DEVICE) was written from outside -- a checkpoint restore,
 * an optimizer of the caller's own: everything the engine derives from Recipe_Embedding / Category_Embedding
 * (retrieval's dish vectors and pattern-grouped tables) is rebuilt on next use.  m2d_train_step and
 * m2d_write_memory do this themselves. */
int m2d_tables_updated(m2d_engine *h);

/* Serving mirror (option "pm_bf16", default 0; a serving option like "user_high_table").  pm_bf16 u16[U, C+1, E] is the bf16 image of
 * Personal_Memory, every value rounded to nearest, ties to even, exactly as torch's float32 -> bfloat16 does it: subnormals are
 * rounded, not flushed; -0 and +-inf are kept; a NaN becomes the quiet NaN 0x7fc0; finite values past the bf16 range become +-inf.
 * The engine builds it on the first call that needs it and again after anything that writes Personal_Memory (m2d_write_memory,
 * m2d_train_step, m2d_tables_updated): one whole pass over the table.  If its allocation fails the call returns M2D_ERR_HIP (text
 * in m2d_last_error); nothing falls back to the f32 table.
 * With the option on, m2d_score_pairs, m2d_score_pairs_bydish, m2d_score_pairs_host and m2d_score_pairs_ingredients read the user
 * rows from the mirror whenever the vectorised C = 4 kernels run -- C = 4, E % 4 == 0, E <= 256, "variant" != 9 -- whatever the
 * batch size.  The scores are the graph's on the rounded table, bit for bit what the f32 kernels return on an engine built from it,
 * NaN and inf positions included; every kernel form ("prefetch", "nt_loads", "skip_masked", "blocks_per_cu", "variant" 11 / 12)
 * returns the same bits.  Against the f32 table a score moves by at most 2^-8 (|a| sum|high-level terms| + |b| sum|low-level
 * terms|) / n.  Because rounding can make an inf the f32 table does not hold, the mirror has a non-finite word of its own:
 * "skip_masked" leaves weight-0 rows out only while that word and the engine's are both clear.  m2d_last_kernel names the f32
 * kernel with "_bf16" behind: m2d_score_pairs_c4_bf16, m2d_score_pairs_c4_small_bf16, m2d_score_pairs_c4_hv_bf16,
 * m2d_score_pairs_c4_small_hv_bf16.  Other shapes (m2d_score_pairs_cn, m2d_score_pairs_generic, "variant" = 9) keep reading the f32
 * table, and m2d_last_kernel says so.  With "user_high_table" = 1 as well the mirror wins: the derived high table is not used, the
 * bits are those of "pm_bf16" alone.
 * NOT affected -- they read the f32 table as before: m2d_rank_candidates (and the evaluator built on it), m2d_topk_users,
 * m2d_catalogue_rank, m2d_topk_users_excluding, the MLP head (m2d_score_pairs_mlp, m2d_topk_users_mlp, m2d_rank_candidates_mlp),
 * m2d_train_step and m2d_write_memory, which read and write the f32 table and make the mirror stale.
 *
 * m2d_pm_bf16 makes the mirror current -- building it if it is stale, whatever the option says -- and copies it into the device
 * buffer `buf` (U (C+1) E halves), on `stream`, without synchronising.  For checkpointing a serving image.  A null pointer is
 * M2D_ERR_INVALID_ARG. */
int m2d_pm_bf16(m2d_engine *h, uint16_t *buf, void *stream);

/* Optimizer steps applied since m2d_train_begin: read (*steps receives it, set = 0) or restored (set = 1, for a
 * checkpoint resume; Adam's bias-correction powers are re-derived from it). */
int m2d_train_steps(m2d_engine *h, int64_t *steps, int32_t set);
int m2d_train_end(m2d_engine *h);

/* ---- build-defined extension, NO reference counterpart (BASELINE.json configs 2-5) ----
 * Multi-hot ingredient table for the high-level path:
 *     H[d]  = sum_j w_j ING[id_j] / sum_j w_j     over dish d's list ids[off[d] .. off[d+1])
 *     high  = <U_high[u], H[d]>                    in place of Model_Recommender.py:67-79
 *     score = a*high + (1-a)*low                   low-level path and blend unchanged (:82-96)
 * With ING = Category_Embedding, ids = 0..C-1 and w = the dish's category mask this is the reference's
 * formula.  ing f32[R, E]; off i32[I+1] (CSR, off[0] = 0); ids i32[nnz]; w f32[nnz] or NULL (all 1).
 * The call gathers and segment-sums the rows into H once (it synchronises and reports a malformed CSR /
 * bad id as M2D_ERR_BAD_INGREDIENT; an id error still latched from an earlier launch is returned first, under its own
 * code, exactly as m2d_check would); all four arrays use `table_flags`.  A dish with an empty list
 * scores NaN, like an empty category mask.  Failures: "Setters" above -- after M2D_ERR_BAD_INGREDIENT or a HIP error there is no
 * ingredient table, as after m2d_clear_ingredients. */
int m2d_set_ingredients(m2d_engine *h, const float *ing, int64_t R, const int32_t *off, const int32_t *ids,
                        const float *w, int64_t nnz, int table_flags);
int m2d_clear_ingredients(m2d_engine *h);

/* m2d_score_pairs with the ingredient high-level path.  cats f32[B, C] feeds the low-level path;
 * cats == NULL uses the resident dish masks (m2d_set_dish_categories). */
int m2d_score_pairs_ingredients(m2d_engine *h, const int32_t *users, const int32_t *items, const float *cats,
                                int64_t B, float *out, void *stream);

/* ---- build-defined extension, NO reference counterpart (BASELINE.json configs[2]) ----
 * 3-layer scoring head on the interaction vector z[k] = flatten(PM[u])[k] * Dt[d][k], k < K = (C+1)*E
 * (sum_k z[k] is the reference score, Model_Recommender.py:67-96 in factored form):
 *     score = sum_k z[k] + w3 . relu(W2^T relu(W1^T z + b1) + b2) + b3
 * W1 f32[K, H1], b1 f32[H1], W2 f32[H1, H2], b2 f32[H2], w3 f32[H2].  H1 = 256, H2 = 64 with K % 64 == 0
 * run on the MFMA kernels (split-bf16 layers 1-2 by default, exact f32 with option "mlp_bf16x3" = 0), and so do
 * K % 4 == 0, K <= 1280 on a W1 copy zero-padded to whole 64-row chunks (the reference's embed_size 200 gives
 * K = 1000); other sizes run a generic kernel.  Dish masks must be resident
 * (m2d_set_dish_categories); the ingredient table, when set, feeds Dt's high-level part.  W1 and W2 are read 16 bytes at a time:
 * borrowed ones must be 16-byte aligned.  Failures: "Setters" above. */
int m2d_set_mlp_head(m2d_engine *h, const float *W1, const float *b1, const float *W2, const float *b2,
                     const float *w3, float b3, int32_t H1, int32_t H2, int table_flags);
int m2d_clear_mlp_head(m2d_engine *h);
int m2d_score_pairs_mlp(m2d_engine *h, const int32_t *users, const int32_t *items, int64_t B, float *out,
                        void *stream);

/* Retrieval and candidate ranking under the head (build-defined, like the head).  The score of a (user, dish) pair is
 * m2d_score_pairs_mlp's in every mode -- the head added to the reference score, masks from the resident dish table, the ingredient
 * table feeding Dt's high-level part when it is set -- and every score comes from that call's launcher, whichever kernel family
 * the shape selects.  The order is m2d_topk_users' applied to those scores: score descending, bit-equal scores and -0 / +0 to the
 * lower dish id, NaN scores last (after every -inf) in id order.  (m2d_topk_users itself ignores the head, as before.)
 *
 * m2d_topk_users_mlp, candidates == 0 (exact): every dish of [0, I) is scored under the head for every listed user; the first k of
 * the order go to out_ids i32[nU, k] / out_scores f32[nU, k].  1 <= k <= min(64, I).  The work runs in chunks of at most
 * "topk_mlp_chunk_pairs" pairs (P): dish ranges of W = min(I, P) dishes, user blocks of max(1, P / W) rows; for each user block, for
 * each dish range: the pairs are written, scored, and m2d_topk_mlp_select merges the range into the rows' running lists (kept in
 * the output buffers).  The lists do not depend on P: same ids, same score bits.
 * m2d_topk_users_mlp, k <= candidates <= min(64, I) (two-stage, K1 = candidates): stage 1 is m2d_topk_users as it runs with default
 * options -- K1 dishes per user by the reference / ingredient score --, stage 2 scores those nU x K1 pairs under the head and returns
 * the first k of the same order among them.  Any other `candidates`: M2D_ERR_INVALID_ARG.
 * m2d_rank_candidates_mlp: m2d_rank_candidates with the segment scores taken from the head; dict collapse, tie order, padding and
 * the NaN flag are that call's, unchanged.
 * No head or no dish masks: M2D_ERR_NOT_CONFIGURED.  A bad user id is latched (m2d_check; the position reported is the pair's inside
 * its chunk), that call's rows are unspecified and the engine stays usable.  m2d_set_user_base is honoured (ids stay global);
 * users may repeat.  Neither call synchronises more than m2d_topk_users / m2d_score_pairs_mlp do; after the first call of a size
 * they allocate only on growth.  Diagnostic: "topk_mlp_launches". */
int m2d_topk_users_mlp(m2d_engine *h, const int32_t *users, int64_t nU, int32_t k, int32_t candidates,
                       float *out_scores, int32_t *out_ids, void *stream);
int m2d_rank_candidates_mlp(m2d_engine *h, const int32_t *users, const int32_t *items, const int32_t *lens,
                            int64_t nseg, int32_t L, int32_t k, float *out_scores, int32_t *out_items,
                            int32_t *out_flags, void *stream);

/* Seen-dish filtering under the head (build-defined, like the head).  Score and order are those above: the pair's
 * m2d_score_pairs_mlp word, score descending, equal bits and -0 / +0 to the lower id, NaN after every -inf in id order.  The
 * exclusion lists follow m2d_catalogue_rank: device CSR, excl_off i64[n + 1], excl_ids i32 of excl_off[n] entries (read on the
 * device), ascending within a segment, equal neighbours allowed and counted once; excl_off == NULL: no exclusions.
 *
 * m2d_topk_users_mlp_excluding, candidates == 0: row i holds the first k of the order over [0, I) less user i's segment, id -1 /
 * NaN from the number of dishes left on (m2d_topk_users_excluding's convention); 1 <= k <= min(64, I).  Chunk geometry, engine
 * buffers and "topk_mlp_launches" are m2d_topk_users_mlp's; the lists do not depend on "topk_mlp_chunk_pairs".
 * k <= candidates <= min(16, I): stage 1 is m2d_topk_users_excluding (K1 = candidates dishes by the reference score, the segment
 * already left out) with that call's conditions -- C = 4, 0/1 masks, finite tables, E a multiple of 4 up to 256, no ingredient
 * table: otherwise M2D_ERR_UNSUPPORTED naming the condition --, stage 2 scores the nU x K1 candidates under the head and lists the
 * first k; a slot stage 1 left empty is dropped.  Any other `candidates` with exclusions: M2D_ERR_INVALID_ARG.
 * excl_off == NULL: the call IS m2d_topk_users_mlp -- its launches, its words, its `candidates` range.
 *
 * m2d_catalogue_rank_mlp: for query i = (u, p) with segment X,
 *     out_rank[i] = #{ d in [0, I), d not in X, d != p : (score(u, d), d) precedes (score(u, p), p) in the order },
 * out_scores[i] (may be NULL) the held-out pair's word; an id of X equal to p is ignored.  For the same u and X,
 * m2d_catalogue_rank_mlp(u, out_ids[u][j], X) == j for every dish the exact mode lists, at every chunk size.
 * "topk_mlp_launches" counts the held-out launch too.
 *
 * Both: no head or no dish masks: M2D_ERR_NOT_CONFIGURED; null buffers, excl_off without excl_ids: M2D_ERR_INVALID_ARG.  Latched
 * (m2d_check): a bad user id (M2D_ERR_BAD_USER_ID), a bad held-out id (M2D_ERR_BAD_ITEM_ID), a bad excluded id (M2D_ERR_BAD_ITEM_ID,
 * its index into excl_ids), an id below its predecessor or an offset below its predecessor / a first offset other than 0
 * (M2D_ERR_INVALID_ARG, its index) -- looked at once per call; a bad excluded id indexes nothing.  A call with a latched error leaves
 * its rows unspecified and the engine usable.  Neither call synchronises; after the first call of a size they allocate only on
 * growth.  m2d_set_user_base is honoured. */
int m2d_topk_users_mlp_excluding(m2d_engine *h, const int32_t *users, int64_t nU, int32_t k, int32_t candidates,
                                 const int64_t *excl_off, const int32_t *excl_ids,
                                 float *out_scores, int32_t *out_ids, void *stream);
int m2d_catalogue_rank_mlp(m2d_engine *h, const int32_t *users, const int32_t *items, int64_t n,
                           const int64_t *excl_off, const int32_t *excl_ids,
                           int32_t *out_rank, float *out_scores, void *stream);

/* ---- build-defined generalisation, NO reference counterpart (like m2d_topk_users) ----
 * Slate scoring: many users against ONE shared list of dishes -- the dishes that can be cooked from today's market, a shared negative
 * pool, an editorial list.  m2d_score_slate writes the whole score matrix, m2d_topk_slate the k best dishes of the slate per user.
 *
 * Inputs.  users i32[nU], device memory, global ids: m2d_set_user_base is honoured, users may repeat.  slate i32[nD], device memory,
 * 1 <= nD <= I, STRICTLY ASCENDING dish ids (the convention of the exclusion lists: "lower column" and "lower dish id" are the same).
 * A slate id outside [0, I) is latched as M2D_ERR_BAD_ITEM_ID with its index, an entry not greater than its predecessor as
 * M2D_ERR_INVALID_ARG with its index, a bad user id as M2D_ERR_BAD_USER_ID with its index in `users`; m2d_check reports them as
 * elsewhere.  The rows of a call with a latched error are unspecified; no kernel reads out of bounds and the engine stays usable.
 * nU == 0 returns M2D_OK and launches nothing.  nD < 1, nD > I, k < 1, k > min(64, nD) or a null pointer: M2D_ERR_INVALID_ARG.
 *
 * Score.  out[i, j] = <flatten(PM[users[i]]), Dt[slate[j]]>, out f32[nU, nD] row-major, Dt[d] computed by exactly the expressions of
 * the full-catalogue dish vectors (Model_Recommender.py:67-96 in factored form: Dt[d] = concat(a (sum_c m_c CE_c) / n,
 * (1 - a) (m_c / n) RE[d] for each c), n = sum_c m_c).  One f32 accumulator per (user, dish) starts at +0 and takes one fused
 * multiply-add per k, in an order of k that depends on E alone: the bits of out[i, j] do not depend on nU, nD, the row's or the
 * column's position, or how the launcher cuts the work.  Masks are the resident dish table (m2d_set_dish_categories; without it
 * M2D_ERR_NOT_CONFIGURED), any float weights; a dish with an empty mask gives a NaN column (0 / 0, as everywhere).
 *
 * m2d_topk_slate returns the first k of m2d_topk_users' order over the slate only -- score descending, bit-equal scores and -0 / +0 to
 * the lower dish id, NaN last in id order -- as out_ids i32[nU, k] (dish ids, not columns) / out_scores f32[nU, k]; a listed score is
 * the word m2d_score_slate writes for that (user, dish), bit for bit.  Users are taken in blocks of max(1, P / nD) rows, P = option
 * "slate_chunk_pairs": a block's scores go to engine scratch and m2d_topk_mlp_select lists them.  The lists do not depend on P.
 *
 * Refused with M2D_ERR_UNSUPPORTED, the condition named in m2d_last_error (m2d_catalogue_rank's precedent): a table value that is not
 * finite (the engine's "a table value is not finite" word), the ingredient table set, an MLP head set.
 *
 * Kernels: m2d_build_slate_vectors writes the slate's dish vectors into engine scratch on every call (the full-catalogue table of
 * m2d_topk_users is neither built nor read); m2d_score_slate_mfma -- C = 4, E a multiple of 4 up to 256 -- is an LDS-tiled contraction
 * on the exact-f32 matrix instruction, m2d_score_slate_generic serves every other shape (and "variant" = 9).  m2d_last_kernel names the
 * scoring kernel.  Neither call synchronises, beyond one read of the not-finite word after a write to the tables (as m2d_topk_users);
 * after the first call of a size they allocate only on growth. */
int m2d_score_slate(m2d_engine *h, const int32_t *users, int64_t nU, const int32_t *slate, int64_t nD,
                    float *out /* f32[nU, nD], row-major */, void *stream);
int m2d_topk_slate(m2d_engine *h, const int32_t *users, int64_t nU, const int32_t *slate, int64_t nD, int32_t k,
                   float *out_scores /* [nU, k] */, int32_t *out_ids /* [nU, k] */, void *stream);

/* ---- build-defined extension, NO reference counterpart ----
 * Deep retrieval lists: full-catalogue top-k for 1 <= k <= min(1024, I), with optional per-user exclusion lists, and the same under the
 * MLP head with up to 1024 first-stage candidates.  Every other retrieval call stops at 64 entries; these two take the same order
 * further (candidate generation for a reranker, HR@100 / recall@500, pagination).
 *
 * m2d_topk_users_deep.  users i32[nU], device memory, global ids (m2d_set_user_base is honoured, users may repeat).  excl_off i64[nU + 1]
 * / excl_ids i32[excl_off[nU]], device memory, or excl_off NULL for none: user i's list leaves out excl_ids[excl_off[i] .. excl_off[i+1]),
 * the conventions of m2d_catalogue_rank (offsets from 0 and non-decreasing, ids of a segment ascending, repeats allowed).  out_ids
 * i32[nU, k] / out_scores f32[nU, k]: the first k of m2d_topk_users' order -- score descending, bit-equal scores and -0 / +0 to the lower
 * dish id, NaN last in id order -- over the dishes not excluded; rows end in id -1 / NaN where fewer than k remain.  A listed score is
 * the word m2d_score_slate writes for that (user, dish), bit for bit; an MLP head, if set, is ignored (as by m2d_topk_users).
 * nU == 0 returns M2D_OK and launches nothing.  k < 1, k > min(1024, I), a null pointer, excl_off without excl_ids:
 * M2D_ERR_INVALID_ARG.  No dish masks: M2D_ERR_NOT_CONFIGURED.  Refused with M2D_ERR_UNSUPPORTED, the condition named in
 * m2d_last_error: the ingredient table set, a table value that is not finite (m2d_topk_slate's rule).
 * Diagnostics.  A bad user id is latched as M2D_ERR_BAD_USER_ID with its index in `users`; an excluded id outside [0, I) as
 * M2D_ERR_BAD_ITEM_ID, an id below its predecessor or an offset that is not 0 at [0] / below its predecessor as M2D_ERR_INVALID_ARG,
 * each with the position m2d_topk_users_excluding reports; m2d_check reports them.  The rows of a call with a latched error are
 * unspecified; no kernel reads out of bounds and the engine stays usable.
 * How.  Dish ranges of W = min(I, P, 65536) dishes, user blocks of max(1, P / W) rows, P = option "deep_chunk_pairs": per block and
 * range m2d_build_slate_vectors (its dish-range form), the slate score kernel into engine scratch, and m2d_select_deep -- a radix
 * select on the order's 64-bit key, one workgroup per row, O(W) for any k -- which starts the row's list on the first range and merges
 * into it on the others.  The lists do not depend on P.  Does not synchronise beyond what m2d_topk_slate does; allocates only on growth.
 *
 * m2d_topk_users_mlp_deep.  m2d_topk_users_mlp_excluding's scores (the pair's m2d_score_pairs_mlp word) and order, 1 <= k <= min(1024, I).
 * candidates == 0: every dish not excluded is scored under the head (m2d_topk_users_mlp's loop and "topk_mlp_chunk_pairs" geometry,
 * m2d_select_deep in place of its selection); works with the ingredient table set.  k <= candidates <= min(1024, I): per block of
 * max(1, P / candidates) users, stage 1 is m2d_topk_users_deep's list of `candidates` dishes for the user and segment -- with its
 * refusals, under this call's name --, stage 2 scores them under the head and lists the first k; a slot stage 1 left empty is dropped.
 * Any other `candidates`: M2D_ERR_INVALID_ARG.  No head or no dish masks: M2D_ERR_NOT_CONFIGURED.  Diagnostics as above. */
int m2d_topk_users_deep(m2d_engine *h, const int32_t *users, int64_t nU, int32_t k,
                        const int64_t *excl_off /* [nU + 1] or NULL */, const int32_t *excl_ids,
                        float *out_scores /* [nU, k] */, int32_t *out_ids /* [nU, k] */, void *stream);
int m2d_topk_users_mlp_deep(m2d_engine *h, const int32_t *users, int64_t nU, int32_t k, int32_t candidates,
                            const int64_t *excl_off /* [nU + 1] or NULL */, const int32_t *excl_ids,
                            float *out_scores /* [nU, k] */, int32_t *out_ids /* [nU, k] */, void *stream);

/* ---- build-defined extension, NO reference counterpart ----
 * Household retrieval: ONE list of dishes for a GROUP of users -- the people at one table.
 *
 * Groups.  members i32[nG, M], device memory, row-major, 1 <= M <= M2D_GROUP_MAX_MEMBERS: group g's members are the leading entries
 * >= 0 of row g, -1 fills the rest of the row; a group has at least one member.  Ids are global (m2d_set_user_base is honoured: EVERY
 * member must lie in this engine's range -- a household spread over several shards is not served, sharding is out of scope) and may
 * repeat; a repeated member counts twice in the mean.
 *
 * Group word.  With s_j the word m2d_score_slate writes for (member j, dish d), `mode` chooses the group's word for d:
 *   M2D_GROUP_LEAST  least misery: the word of the member that ranks worst under m2d_topk_users' order -- the lowest score, -0 and +0
 *                    equal, NaN worst; among equals the first in member order;
 *   M2D_GROUP_MOST   the word of the member that ranks best (first member among equals); NaN only if every member's word is NaN;
 *   M2D_GROUP_MEAN   acc = s_0; acc = acc + s_j for j = 1 .. cnt - 1 in member order, float32, round to nearest; then one correctly
 *                    rounded float32 division by (float)cnt (cnt >= 2).  No fma, no reciprocal, no pairwise tree.
 * With one member every mode returns that member's word: a group of one reproduces m2d_topk_users_deep bit for bit.  A group word
 * does not depend on nG, the group's position in the call, M (the padding) or how the launcher cuts the work.
 *
 * m2d_topk_groups: the first k of m2d_topk_users' order on the group words over the whole catalogue, 1 <= k <= min(1024, I), as
 * out_ids i32[nG, k] / out_scores f32[nG, k]; optional per-group exclusion lists excl_off i64[nG + 1] / excl_ids in m2d_catalogue_rank's
 * conventions (excl_off NULL: none); rows end in id -1 / NaN where fewer than k dishes remain.
 * m2d_score_groups_slate / m2d_topk_groups_slate: the group words of a slate -- m2d_topk_slate's slate: strictly ascending, 1 <= nD <= I,
 * the same latched errors -- as out f32[nG, nD], or their first k, 1 <= k <= min(1024, nD), as dish ids (not columns).  The slate forms
 * take no exclusion lists: the caller takes the ids out of the slate.
 *
 * nG == 0 returns M2D_OK and launches nothing.  M, mode or k out of range, a null required pointer, excl_off without excl_ids:
 * M2D_ERR_INVALID_ARG.  No dish masks: M2D_ERR_NOT_CONFIGURED.  Refused with M2D_ERR_UNSUPPORTED under the call's own name, the condition
 * in m2d_last_error: the ingredient table set, a table value that is not finite (m2d_topk_users_deep's conditions; an MLP head is ignored).
 * Diagnostics (latched, first error wins; the member check runs first in stream order).  A member id that is neither -1 nor in the
 * engine's range -- an entry below -1 included -- M2D_ERR_BAD_USER_ID with the id and its position g M + j in `members`; an empty group
 * M2D_ERR_INVALID_ARG with value -1 and position g M; an id >= 0 behind a -1 M2D_ERR_INVALID_ARG with the id and its position;
 * exclusion errors as m2d_topk_users_deep reports them.  A row with several defects (-1, id: an empty group AND an id behind a -1) has
 * ONE of them reported, whichever thread latches first.  The rows of a call with a latched error are unspecified; no kernel reads out
 * of bounds and the engine stays usable.
 * How.  m2d_group_members checks the slots and writes a dense array of valid user ids and each group's count; per block of
 * Gb = max(1, P / (M W)) whole groups (P = option "deep_chunk_pairs") and dish range of W = min(I, P, 65536) dishes (slate forms:
 * W = nD, one range) the slate score kernel fills engine scratch [Gb M, W], m2d_group_reduce folds each group's first cnt rows into its
 * row 0 (m2d_score_groups_slate: into `out`), and m2d_select_deep lists row 0 of every group, merging across ranges as m2d_topk_users_deep
 * does.  The slate forms do not cut the slate into ranges: their scratch is at least M nD floats whatever the option says (M = 64 and
 * nD = 10^6: 256 MB).  KNOWN COST: filler rows are scored too, so the scoring cost grows with the padding M - cnt; compaction is not done here.
 * Does not synchronise beyond what m2d_topk_slate does; buffers grow only. */
#define M2D_GROUP_LEAST 0
#define M2D_GROUP_MEAN 1
#define M2D_GROUP_MOST 2
#define M2D_GROUP_MAX_MEMBERS 64
int m2d_topk_groups(m2d_engine *h, const int32_t *members /* [nG, M] */, int64_t nG, int32_t M, int32_t mode, int32_t k,
                    const int64_t *excl_off /* [nG + 1] or NULL */, const int32_t *excl_ids,
                    float *out_scores /* [nG, k] */, int32_t *out_ids /* [nG, k] */, void *stream);
int m2d_score_groups_slate(m2d_engine *h, const int32_t *members /* [nG, M] */, int64_t nG, int32_t M, int32_t mode,
                           const int32_t *slate, int64_t nD, float *out /* f32[nG, nD], row-major */, void *stream);
int m2d_topk_groups_slate(m2d_engine *h, const int32_t *members /* [nG, M] */, int64_t nG, int32_t M, int32_t mode,
                          const int32_t *slate, int64_t nD, int32_t k,
                          float *out_scores /* [nG, k] */, int32_t *out_ids /* [nG, k] */, void *stream);

/* ---- build-defined extension, NO reference counterpart ----
 * Menu retrieval: the k best dishes of the whole catalogue with AT MOST caps[u][c] DISHES OF CATEGORY c in user u's list.
 *
 * Membership.  Dish d is in category c iff cats[d][c] != 0.0f in C semantics, cats the table of m2d_set_dish_categories: -0.0 is no
 * member, any other word is one (weighted masks, negative weights, a NaN weight).  sig(d) is the C-bit mask of d's categories.
 * C <= M2D_MENU_MAX_CATEGORIES = 6: at most 64 signatures, one per lane of a wave.
 *
 * Menu of user u.  Walk all I dishes in m2d_topk_users' order -- score descending, bit-equal scores and -0 / +0 to the lower dish id, NaN
 * last in id order; the score is the word m2d_score_slate writes for (u, d) -- with a count n[c] = 0 per category: dish d is taken iff
 * n[c] < caps[u][c] for every c in sig(d); taking it adds 1 to n[c] for each of them; the walk stops at k dishes.  A dish with an empty
 * mask is in no category and is never capped (its score is NaN: it comes last).  Rows end in id -1 / NaN where fewer than k dishes can
 * be taken.  With every cap >= k the row is m2d_topk_users_deep's list for that user, bit for bit.
 *
 * m2d_topk_menu.  users i32[nU], device memory, global ids (m2d_set_user_base is honoured, users may repeat); caps i32[nU, C], device
 * memory, row-major, one row per entry of `users`; 1 <= k <= min(64, I); out_ids i32[nU, k] / out_scores f32[nU, k].  nU == 0 returns
 * M2D_OK and launches nothing.  A null pointer or k out of range: M2D_ERR_INVALID_ARG.  No dish masks: M2D_ERR_NOT_CONFIGURED.  Refused
 * with M2D_ERR_UNSUPPORTED under the call's own name, the condition in m2d_last_error: C > 6, the ingredient table set, a table value
 * that is not finite (m2d_topk_users_deep's conditions; an MLP head is ignored).
 * Diagnostics (latched, first error wins; m2d_check reports them).  A bad user id: M2D_ERR_BAD_USER_ID with its index in `users`; a cap
 * below 0: M2D_ERR_INVALID_ARG with the cap as value and u * C + c as position.  The rows of a call with a latched error are
 * unspecified; no kernel reads or writes out of bounds and the engine stays usable.
 * The lists do not depend on option "deep_chunk_pairs", on nU, on the row's position or on how the launcher cuts the work.
 * How.  The menu over the full order equals the menu over the merge of each signature's own first k dishes (a category at its cap
 * stays there, so a signature that stops being admissible never returns).  The signature index -- the dish ids sorted by
 * (signature, id) and 65 segment offsets -- is built by the first call after the masks were set or changed (m2d_set_dish_categories,
 * m2d_tables_updated): three launches, no sort, and ONE STREAM SYNCHRONISATION that reads the 64 segment sizes to the host.  After
 * that a call synchronises no more than m2d_topk_slate does and allocates only on growth: per block of users and non-empty segment,
 * ranges of W = min(segment size, P, 65536) dishes (P = option "deep_chunk_pairs") are scored as slates into engine scratch and
 * listed (option "menu_select") into list scratch [segments, users of a block, k]; m2d_menu_merge, one wave per user with lane s
 * holding the cursor into signature s's list, then takes the best admissible head k times.  User blocks keep the score scratch and
 * the list scratch within P words each.
 * Not offered here: per-user exclusion lists and slates (`among`) -- m2d_topk_menu_filtered below takes both --; nowhere: minimum
 * quotas, the MLP head, k above 64. */
#define M2D_MENU_MAX_CATEGORIES 6
int m2d_topk_menu(m2d_engine *h, const int32_t *users /* device [nU] */, int64_t nU, int32_t k,
                  const int32_t *caps /* device [nU, C] */,
                  float *out_scores /* [nU, k] */, int32_t *out_ids /* [nU, k] */, void *stream);

/* ---- build-defined extension, NO reference counterpart ----
 * Menu retrieval over a slate or market, with per-user exclusions: m2d_topk_menu's greedy walk over the dishes of `slate` (all I dishes
 * when slate == NULL), less user u's exclusion segment.  A dish that is left out counts against no cap; listed scores are
 * m2d_score_slate's words; rows end in id -1 / NaN where fewer than k dishes can be taken.
 *
 * Arguments.  users, caps, the outputs: as m2d_topk_menu.  excl_off i64[nU + 1] / excl_ids i32[excl_off[nU]], device memory, by
 * m2d_catalogue_rank's conventions (offsets from 0 and non-decreasing, a segment's ids ascending, repeats allowed); an excluded id that
 * is not in the slate is ignored.  slate i32[nD], device memory, STRICTLY ASCENDING dish ids, 1 <= nD <= I.  1 <= k <= min(64, I)
 * whatever nD is.  nU == 0 returns M2D_OK and launches nothing.  nD out of range with a slate, excl_off without excl_ids, a null
 * required pointer, k out of range: M2D_ERR_INVALID_ARG.  Refusals are m2d_topk_menu's, under this call's name.
 * Diagnostics (latched, first error wins).  Exclusion lists are checked as m2d_topk_users_deep checks them: the same codes, values and
 * positions.  A slate id outside [0, I): M2D_ERR_BAD_ITEM_ID with the id and its index in `slate`; a slate entry not above its
 * predecessor: M2D_ERR_INVALID_ARG with the entry and its index (m2d_topk_slate's convention; both checks run before any scoring
 * launch in stream order).  Bad users and caps below 0 as m2d_topk_menu.  The rows of a call with a latched error are unspecified; ids
 * are only ever compared, so no kernel reads or writes out of bounds whatever the lists hold, and the engine stays usable.
 * With excl_off == NULL and slate == NULL the call IS m2d_topk_menu: the same launches, the same words.  The lists do not depend on
 * options "deep_chunk_pairs" and "menu_select", on nU or on the row's position.
 * How.  Removing dishes from the order leaves m2d_topk_menu's identity intact: the menu over the allowed order is the menu over the
 * merge of each signature's first k ALLOWED dishes.  Exclusions: a range of a signature's segment is an ascending id table, a row's
 * exclusion segment is ascending, and the selection strikes one against the other with a forward-only cursor (a window between the
 * lower bounds of the ids under a step's first and last column; one scalar compare where it is empty).  Slate: the slate is
 * partitioned by signature with the index's three passes, the flag pass reading the catalogue index's resident signature bytes (so that
 * index is built first, as m2d_topk_menu builds it) -- and the 64 segment sizes are read to the host: ONE STREAM SYNCHRONISATION PER
 * CALL WITH A SLATE.  Without a slate the call synchronises as m2d_topk_menu does.  Scratch lives in engine buffers that grow only.
 * Not offered: minimum quotas, the MLP head, sharding, k above 64, C above 6. */
int m2d_topk_menu_filtered(m2d_engine *h, const int32_t *users /* device [nU] */, int64_t nU, int32_t k,
                           const int32_t *caps /* device [nU, C] */,
                           const int64_t *excl_off /* [nU + 1] or NULL */, const int32_t *excl_ids,
                           const int32_t *slate /* [nD] strictly ascending, or NULL: the whole catalogue */, int64_t nD,
                           float *out_scores /* [nU, k] */, int32_t *out_ids /* [nU, k] */, void *stream);

/* ---- build-defined extension, NO reference counterpart ----
 * Meal plans: `days` menus of k dishes per user with no dish twice, every day under caps[u][c] and the whole plan under plan_caps[u][c]
 * dishes of category c -- in one call, with one scoring pass.
 *
 * Definition.  Day 1 is m2d_topk_menu_filtered's row.  Day d is that call with the dishes of days 1 .. d - 1 added to user u's
 * exclusions and with the caps min(caps[u][c], plan_caps[u][c] - the dishes of category c listed on earlier days), floored at 0.
 * out_ids i32[nU, days, k] / out_scores f32[nU, days, k]: each row of [days, k] ends in id -1 / the fill NaN where the day cannot take
 * k dishes, and every row is written.  A day that takes nothing is followed by days that take nothing.
 *
 * Arguments.  1 <= k <= min(64, I); days >= 1; days * k <= M2D_PLAN_MAX_LIST = 1024 (days * k may exceed I or nD).  caps i32[nU, C] per
 * day; plan_caps i32[nU, C] over the plan, or NULL: none.  users, excl_off / excl_ids, slate / nD: as m2d_topk_menu_filtered, and so
 * are the refusals, the list checks, the slate check and bad users, under this call's name.  days or days * k out of range:
 * M2D_ERR_INVALID_ARG.
 * Diagnostics.  A cap below 0: M2D_ERR_INVALID_ARG with the cap and position u * C + c; a plan cap below 0: the same with position
 * nU * C + u * C + c (the two tables as one array, caps first).  Either counts as 0.
 * The words are m2d_score_slate's; the rows do not depend on options "deep_chunk_pairs" and "menu_select", on nU or on the row's
 * position.  With days == 1 and plan_caps == NULL the call IS m2d_topk_menu_filtered: the same launches, the same words.
 * How.  m2d_menu_merge moves a signature's cursor only when it takes the entry under it, so whatever the caps do the dishes a walk takes
 * from a signature are a PREFIX of that signature's own order.  Day d + 1 over the order less what days 1 .. d took is therefore the
 * same walk with the cursors where day d left them and the day counts back at 0; a plan takes at most days * k dishes, so it never
 * reaches past a signature's first L = days * k allowed dishes.  The launcher is m2d_topk_menu_filtered's with lists of L (list
 * scratch [segments, users of a block, L]; user blocks of max(1, P / max(W, segments * L)) rows; above L = 64 the selection is
 * m2d_select_deep whatever "menu_select" says), and m2d_plan_merge -- one wave per user, lane s holding signature s's cursor and a
 * window of its next 8 entries in registers, refilled by independent loads -- runs the days: `full` is the categories at their day
 * cap (back the next morning) or at their plan cap (never back).  One scoring pass instead of `days`.
 * Not offered: per-day cap tables, minimum quotas, the MLP head, sharding, k above 64, C above 6 (households: m2d_plan_groups below). */
#define M2D_PLAN_MAX_LIST 1024
int m2d_plan_menus(m2d_engine *h, const int32_t *users /* device [nU] */, int64_t nU, int32_t days, int32_t k,
                   const int32_t *caps /* device [nU, C]: per day */,
                   const int32_t *plan_caps /* device [nU, C] or NULL: over the whole plan */,
                   const int64_t *excl_off /* [nU + 1] or NULL */, const int32_t *excl_ids,
                   const int32_t *slate /* [nD] strictly ascending, or NULL: the whole catalogue */, int64_t nD,
                   float *out_scores /* [nU, days, k] */, int32_t *out_ids /* [nU, days, k] */, void *stream);

/* ---- build-defined extension, NO reference counterpart ----
 * Household meal plans: m2d_plan_menus for GROUPS of users -- `days` menus of k dishes per group, no dish twice, under caps per day and
 * over the plan, the dishes ordered by the group's word under `mode`.  A household menu is days == 1.
 *
 * Definition.  Let w(g, d) be the word m2d_score_groups_slate gives group g for dish d under `mode`.  Row g of the result is
 * m2d_plan_menus' row for a "user" whose score words are w(g, .): the same order (score descending, equal words and -0 / +0 to the lower
 * id, NaN last), the same day caps, plan caps, exclusions (one segment per GROUP) and slate; a short day ends in id -1 / the fill NaN and
 * every row of out_ids i32[nG, days, k] / out_scores f32[nG, days, k] is written.
 *
 * Caps.  caps_per_member == 0: caps and plan_caps are i32[nG, C], one row per group, passed on as they are; a cap below 0 is latched by
 * the merge as in m2d_plan_menus with nG in place of nU (position g C + c, a plan cap nG C + g C + c) and counts as 0.
 * caps_per_member == 1: both are i32[nG, M, C], one row per member SLOT; the group's cap for category c is the MINIMUM over the group's
 * first cnt[g] members of max(cap, 0).  The rows of filler slots are never read: they may hold anything, bind nothing and latch
 * nothing.  A cap below 0 of a real member: M2D_ERR_INVALID_ARG with the cap and position (g M + j) C + c; a plan cap below 0: position
 * nG M C + (g M + j) C + c.  Either counts as 0.  plan_caps == NULL: none, in both forms.
 *
 * Arguments.  members i32[nG, M] / M / mode: as m2d_topk_groups, with its latched member errors by code, value and position (every
 * member must lie in this engine's user_base range: sharding is out of scope).  1 <= k <= min(64, I), days >= 1,
 * days * k <= M2D_PLAN_MAX_LIST, excl_off i64[nG + 1] / excl_ids, slate / nD, the list checks, the slate check, the refusals and the table
 * conditions: as m2d_plan_menus, under this call's name.  caps_per_member other than 0 / 1, a null required pointer:
 * M2D_ERR_INVALID_ARG.  nG == 0 returns M2D_OK and launches nothing.  The member check is the first launch in stream order and the cap
 * fold the second, so their latches come before any other.  The rows of a call with a latched error are unspecified; no kernel reads
 * or writes out of bounds and the engine stays usable.
 *
 * Invariants.  A row does not depend on options "deep_chunk_pairs" and "menu_select", on nG or the group's position, on M (the
 * padding), or on member order -- except the first-member rule among equal words (LEAST / MOST return that member's word: -0 / +0 and
 * NaN payloads can differ) and the sequential float32 sum of MEAN.
 * Equalities.  A group of one member returns m2d_plan_menus' row for that user in every mode, ids and score words.  With every cap
 * >= days * k and days == 1 the row is m2d_topk_groups' list of k (with a slate: m2d_topk_groups_slate's).  last_kernel is
 * m2d_plan_merge, or m2d_menu_merge when days == 1 and plan_caps == NULL, as in m2d_plan_menus.
 *
 * How.  The prefix argument of m2d_plan_menus speaks of a row's score words only, so it holds for group words unchanged.
 * m2d_group_members checks the slots and writes dense member ids and counts; m2d_group_caps (caps_per_member == 1; one thread per group
 * and category walking the group's cnt rows, both tables) writes the folded, clamped tables into engine scratch, so the merge latches
 * nothing on them.  Then m2d_plan_menus' loop with a group per row: per block of Gb whole groups, non-empty signature segment and range
 * of W = min(segment size, P, 65536) dishes (P = option "deep_chunk_pairs") -- m2d_slate_prepare, the slate score kernel over the
 * block's Gb M member rows into scratch [Gb M, W], m2d_group_reduce in place into each group's row 0, the selection over row 0 with row
 * stride M W, k = L = days * k and the group's exclusion segment; then m2d_plan_merge (m2d_menu_merge when days == 1 without plan
 * caps) over the block.  Blocks outside, ranges inside -- not m2d_topk_groups' order: a block's lists live in list scratch
 * [segments, Gb, L] until its merge, so the other order would need every group's lists at once; a range's dish vectors are therefore
 * rebuilt per block.  Gb = max(1, P / max(M W, segments * L)).  At one group per block the scratch is NOT bounded by the option: M W
 * floats of scores (M = 64, W = 65 536: 16 MB) and segments * L list entries (64 * 1024 * 8 bytes) -- m2d_topk_groups has the same M W
 * caveat.  KNOWN COST: filler rows are scored, as in m2d_topk_groups; no compaction.  Synchronises where m2d_plan_menus does -- the index
 * build once per mask table, once per call with a slate -- and nowhere else; buffers grow only.
 * Not offered: minimum quotas, per-day cap tables, the MLP head, sharding, k above 64, C above 6, member compaction. */
int m2d_plan_groups(m2d_engine *h, const int32_t *members /* device [nG, M], -1 padded */, int64_t nG, int32_t M, int32_t mode,
                    int32_t days, int32_t k,
                    const int32_t *caps, const int32_t *plan_caps /* or NULL */, int32_t caps_per_member,
                    const int64_t *excl_off /* [nG + 1] or NULL */, const int32_t *excl_ids,
                    const int32_t *slate /* strictly ascending or NULL */, int64_t nD,
                    float *out_scores /* [nG, days, k] */, int32_t *out_ids /* [nG, days, k] */, void *stream);

/* Diagnostic (scripts/deep_time.py): one selection launch over a resident row-major score block f32[rows, W], ids 0 .. W - 1, no
 * exclusions, into out_scores / out_ids [rows, k] -- form 0: m2d_select_deep (k <= 1024), form 1: m2d_topk_mlp_select (k <= 64).
 * Reads no table.  Bad arguments: M2D_ERR_INVALID_ARG. */
int m2d_select_probe(m2d_engine *h, const float *scores /* device */, int64_t rows, int64_t W, int32_t k, int32_t form,
                     float *out_scores, int32_t *out_ids, void *stream);

/* ---- build-defined extension, NO reference counterpart ----
 * Market retrieval: from the ingredients seen at the market to the dishes that can be cooked from them -- the slate the calls above
 * were written for.  m2d_set_recipes makes every dish's ingredient list resident, m2d_cookable_dishes turns a market into the
 * ascending list of cookable dishes, which m2d_score_slate / m2d_topk_slate take as it stands.
 *
 * Recipe lists.  off i32[I+1], ids i32[nnz]: dish d's list is ids[off[d] .. off[d+1]), ingredient ids in [0, R), repeats allowed,
 * any order.  R >= 1; nnz = 0 is legal (nothing is ever cookable).  Lists only: no embedding table, no weights.  They are separate
 * from m2d_set_ingredients -- setting or clearing one never touches the other, no scoring call reads the recipes, and the recipes
 * do not make m2d_score_slate / m2d_topk_slate refuse.  `flags`: M2D_TABLES_DEVICE borrows both arrays (they must stay valid and
 * unchanged), M2D_TABLES_HOST copies them.  The call validates once and synchronises, as m2d_set_ingredients does: offsets that are
 * not a CSR row pointer (off[0] = 0, non-decreasing, off[I] = nnz) and an id outside [0, R) (value and position in m2d_last_error)
 * return M2D_ERR_BAD_INGREDIENT and leave the recipes UNSET, and so does a HIP error met on the way (under M2D_ERR_HIP, its own
 * text kept).  A call refused BEFORE anything is replaced leaves the previous recipes set and served, its borrowed arrays still
 * borrowed: M2D_ERR_INVALID_ARG (below), and an id error still latched from an earlier launch, which is returned first, under its
 * own code ("Setters" above).  No later kernel range-checks a recipe id.  A second m2d_set_recipes replaces the first; m2d_clear_recipes
 * returns the engine to "not configured"; m2d_destroy frees owned copies.  R > INT32_MAX, nnz > INT32_MAX, a null pointer or bad
 * flags: M2D_ERR_INVALID_ARG.
 *
 * m2d_cookable_dishes.  Dish d is cookable iff its list is non-empty and the number of its list ENTRIES whose id is not in the
 * market is <= max_missing -- every occurrence counts, an id listed twice and absent counts twice.
 * market i32[nM], device memory: ingredient ids in any order, repeats allowed, nM = 0 allowed (market may then be null).  A market
 * id outside [0, R) is latched as M2D_ERR_BAD_INGREDIENT with its value and index and contributes nothing.  max_missing < 0,
 * nM < 0 or a null out_ids / out_count: M2D_ERR_INVALID_ARG.  No recipes set: M2D_ERR_NOT_CONFIGURED.
 * out_ids i32, device memory, capacity I: out_ids[0 .. count) receives the cookable dishes in STRICTLY ASCENDING order;
 * out_ids[count .. I) is not written.  out_missing i32[I], device memory, may be null: the missing-entry count of EVERY dish, -1 for
 * an empty list.  *out_count (HOST memory) receives count.
 * THE CALL SYNCHRONISES `stream` ONCE, for the count; everything else is stream-ordered.  Because it waits anyway it reads the
 * id-error latch in the same wait and returns what m2d_check would (and clears the latch): a bad market id comes back from this
 * call as M2D_ERR_BAD_INGREDIENT -- the outputs are then those of the market without the bad ids -- and an error latched by an
 * earlier, unchecked launch comes back under its own code.
 *
 * Kernels, in engine scratch that grows on demand: the market as a bitmap of R bits (a memset, then m2d_market_bitmap: atomicOr on
 * 32-bit words); m2d_market_flag, in which a wave owns 64 consecutive dishes -- one contiguous run of `ids`, read coalesced 64 entries
 * a batch, the bitmap in LDS up to 65 536 bits (m2d_market_flag_lds) and read through L2 beyond (m2d_market_flag_l2) -- and writes
 * missing[d] and one kept-count per block of 256 dishes; m2d_market_scan, the exclusive scan of those counts; m2d_market_write, in
 * which every block ranks its kept dishes and stores their ids from its base on.  The order is fixed by construction: no atomic
 * cursor, no sort, and no block waits for another -- four launches give the ordering.  m2d_last_kernel names the flag kernel. */
int m2d_set_recipes(m2d_engine *h, int64_t R, const int32_t *off /* [I+1] */, const int32_t *ids /* [nnz] */, int64_t nnz,
                    int32_t flags);
int m2d_clear_recipes(m2d_engine *h);
int m2d_cookable_dishes(m2d_engine *h, const int32_t *market /* device, [nM] */, int64_t nM, int32_t max_missing,
                        int32_t *out_ids /* device, capacity I */, int32_t *out_missing /* device, [I], may be null */,
                        int64_t *out_count /* HOST */, void *stream);

/* ---- build-defined extension, NO reference counterpart ----
 * Market requests: one user, one market PER REQUEST -- the shape a server meets, many shoppers at once, each with the ingredients seen
 * at their own stall.  m2d_topk_markets filters, scores and lists nQ such requests in one stream-ordered call.  Request q is
 * (users[q], market_ids[market_off[q] .. market_off[q+1])).
 *
 * Cookable set.  Dish d is cookable for request q by m2d_cookable_dishes' definition: its list is non-empty and at most max_missing
 * of its list ENTRIES, every occurrence counted, name an id that is not in the request's market.  Market ids in any order, repeats
 * allowed, an empty market legal (market_ids may be null when nnzM == 0).
 *
 * Outputs.  Row q of out_ids i32[nQ, k] / out_scores f32[nQ, k]: the first min(k, count_q) cookable dishes of request q in
 * m2d_topk_users' order -- score descending, bit-equal scores and -0 / +0 to the lower id, NaN last in id order --, NaN / -1 from
 * column count_q on.  out_counts i32[nQ] (may be null): count_q, the number of COOKABLE dishes, not of listed ones.
 *
 * Score.  A listed score is the literal pair arithmetic's (Model_Recommender.py:67-96 as written, one wave per pair) for (user, dish,
 * the dish's resident mask): bit for bit the word m2d_score_pairs_bydish returns under "variant" = 9, and the way m2d_topk_users'
 * literal kernel defines its scores.  Rows of weight-0 categories are left out as the pair kernels decide it: option "skip_masked" and
 * the engine's "a table value is not finite" word, after the queued table scan has run.  So on tables that hold inf / NaN the call
 * returns the graph's answer (+inf first, -inf after every finite score, NaN last) instead of refusing, and on finite tables the bits do
 * not depend on the option.
 *
 * THE CALL NEVER SYNCHRONISES: everything is stream-ordered, errors are latched for m2d_check, and after the first call of a size it
 * allocates only on growth.  A row's words do not depend on nQ, on the request's position, or on how the launcher cuts the work.
 *
 * Errors.  nQ < 0, nnzM < 0, k < 1, k > 64, max_missing < 0 or a null required pointer: M2D_ERR_INVALID_ARG.  nQ == 0: M2D_OK, nothing
 * launched.  No recipes or no dish masks set: M2D_ERR_NOT_CONFIGURED.  The ingredient table or an MLP head set: M2D_ERR_UNSUPPORTED, the
 * condition named (the refusals of m2d_topk_slate).  Latched, first error wins: a market id outside [0, R) as M2D_ERR_BAD_INGREDIENT
 * with its value and its index in market_ids -- the id contributes nothing; a user id outside the engine's range as
 * M2D_ERR_BAD_USER_ID with its value and q -- that row is all NaN / -1, its count is still the market's, nothing is read for that
 * user; a segment with market_off[q+1] < market_off[q] or one that reaches outside [0, nnzM] as M2D_ERR_INVALID_ARG with
 * market_off[q+1] and q -- the segment is clamped into [0, nnzM] before anything is read.  No kernel reads out of bounds and the
 * engine stays usable.
 *
 * Kernels.  m2d_markets_topk: a block of four waves serves one (request, share), a share being a contiguous range of 256-dish blocks
 * of the catalogue.  The block sets its market's bits in a bitmap -- in LDS up to R = 65 536 (m2d_markets_topk_lds, 8 KiB a block; LDS
 * atomicOr); beyond, a memset and m2d_markets_bitmap write one bitmap of ceil(R / 32) words PER REQUEST into engine scratch in front
 * of it and the block reads its own through L2 (m2d_markets_topk_l2: nQ ceil(R / 32) words of scratch, grown on demand) --, its waves
 * walk the share's 64-dish groups as m2d_market_flag does, score each kept dish with the whole wave and keep the k best as a sorted
 * list across lanes; the four lists meet in LDS (3 KiB).  S = clamp(4 num_cu / nQ, 1, min(64, ceil(I / 256))) shares per request
 * ("market_shares" forces it): with S = 1 the block writes the row, with S > 1 it writes its k (score, id) words into scratch
 * [nQ, S k], adds its count into out_counts (zeroed in front; an integer sum) and m2d_topk_mlp_select merges the shares.  The order is
 * strict, so the words do not depend on S.  m2d_last_kernel names the form. */
int m2d_topk_markets(m2d_engine *h, const int32_t *users /* device, [nQ] */, int64_t nQ,
                     const int64_t *market_off /* device, [nQ + 1] */,
                     const int32_t *market_ids /* device, [nnzM], may be null when nnzM == 0 */, int64_t nnzM,
                     int32_t k, int32_t max_missing, float *out_scores /* device, [nQ, k] */,
                     int32_t *out_ids /* device, [nQ, k] */, int32_t *out_counts /* device, [nQ], may be null */,
                     void *stream);

/* ---- build-defined extension, NO reference counterpart ----
 * m2d_topk_markets with two additions: dishes the shopper has already had are left out, and for every listed dish the call names the
 * list entries its market lacks.  Everything not said here is m2d_topk_markets' rule: the cookable definition, the order, the literal pair
 * score bit for bit, non-finite tables, the refusals, "never synchronises".
 *
 * Exclusions.  X_q = excl_ids[excl_off[q] .. excl_off[q+1]): dish ids, ascending within a segment, repeats count once
 * (m2d_catalogue_rank's conventions; excl_off == NULL: no exclusions).  Row q is the first k of the order over {cookable for q} \ X_q,
 * out_counts[q] the size of that set -- what could be listed, not what is cookable.  An excluded dish is never scored; one that is not
 * cookable has no effect.  With excl_off == NULL and out_missing == NULL every output word equals m2d_topk_markets' (the same kernels
 * are launched).
 *
 * Missing entries.  out_missing i32[nQ, k, max_missing] (may be null; ignored when max_missing == 0): for the listed dish
 * out_ids[q, j] the ingredient ids of its list ENTRIES that are absent from market q, in list order, every occurrence (an id listed twice
 * and absent appears twice), -1 from the number missing on, and all -1 where the id is -1.  Every word is written.  The number of
 * non-negative words equals m2d_cookable_dishes' out_missing for that dish and market.
 *
 * Errors.  Arguments: those of m2d_topk_markets.  excl_ids carries no length: as in m2d_catalogue_rank it is excl_off[nQ], read on the
 * device (0 when excl_ids is NULL).  Latched, first wins: an excluded id outside [0, I) as M2D_ERR_BAD_ITEM_ID with its value and its
 * index in excl_ids; an excluded id below its predecessor in the segment as M2D_ERR_INVALID_ARG with its value and index in excl_ids; a
 * segment with excl_off[q+1] < excl_off[q] or one that reaches outside [0, excl_off[nQ]] -- any non-empty segment when excl_ids is NULL
 * -- as M2D_ERR_INVALID_ARG with excl_off[q+1] and q + 1, its index in excl_off.  Segments are clamped into the array before anything is
 * read, no kernel reads out of bounds; rows of a call with a latched error are unspecified, every other request's row is right.
 *
 * Kernels.  m2d_markets_topk<LDS, true> (m2d_last_kernel: m2d_markets_topk_excl_lds / _l2): per 64-dish group two wave-uniform lower
 * bounds give the segment's window for [d0, d0 + 64); an empty window costs nothing more, otherwise each lane searches the window for
 * its own dish and the result leaves the kept ballot before the scoring loop.  The share-0 block of a request validates its segment
 * once.  m2d_markets_missing, after the rows are final (after the share merge when S > 1): one block per request with the request's
 * bitmap (rebuilt in LDS, or the one left in scratch by the through-L2 form), a wave per listed dish, 64 entries a batch, each absent
 * entry placed by the ballot's popcount below its lane plus the running total -- list order by construction, writes capped at
 * max_missing. */
int m2d_topk_markets_excluding(m2d_engine *h, const int32_t *users /* device, [nQ] */, int64_t nQ,
                               const int64_t *market_off /* device, [nQ + 1] */,
                               const int32_t *market_ids /* device, [nnzM], may be null when nnzM == 0 */, int64_t nnzM,
                               const int64_t *excl_off /* device, [nQ + 1], NULL = no exclusions */,
                               const int32_t *excl_ids /* device, [excl_off[nQ]] */,
                               int32_t k, int32_t max_missing, float *out_scores /* device, [nQ, k] */,
                               int32_t *out_ids /* device, [nQ, k] */, int32_t *out_counts /* device, [nQ], may be null */,
                               int32_t *out_missing /* device, [nQ, k, max_missing], may be null */, void *stream);

/* ---- build-defined extension, NO reference counterpart: serving from health labels ----
 * The reference reads General_Memory only while it writes (Write_Memory, Model_Recommender.py:170-198: PM[u] += alpha * g, g the
 * label-weighted mean of General_Memory's rows).  A profile is that row BY VALUE, nothing is written: q = (u_q, y_q), y_q the f32[L]
 * user_one_hot_label row (any non-negative weights), u_q a user id or -1 for a guest (users == NULL: every request is a guest).
 * In float32, in this order (label order, labels of weight 0 are not read):
 *     ysum = sum_l y_l                     plain adds
 *     g_k  = fmaf(y_l, GM[l][k], g_k)      from 0
 *     M_k  = base_k + alpha * (g_k / ysum) true division, one rounded product, one rounded sum (not fused)
 *     base = PM[u_q - user_base] for u_q >= 0, zeros for a guest
 * -- m2d_write_memory's own g, ysum and alpha * (g / ysum) followed by the add its atomic performs: for distinct known users the row
 * equals Personal_Memory[u] after m2d_write_memory(which = PERSONAL, beta_1 = beta_2 = 0) bit for bit.
 *
 * Containment.  While the engine's tables are finite, a request whose row would hold an inf / NaN (ysum == 0, an inf / NaN in an
 * ADDRESSED General_Memory row, overflow) gets a row of zeros and latches M2D_ERR_INVALID_ARG with bad_value = its number of non-zero
 * labels and bad_index = q; once a table value is not finite the rows are written as computed and retrieval takes the literal
 * kernels, as it does for users.  u_q outside the table and not -1: a row of zeros, M2D_ERR_BAD_USER_ID with (u_q, q).  Rows of a
 * request with a latched error are otherwise unspecified; the call always completes, m2d_check reports.
 *
 * m2d_compose_profiles writes the rows.  The three serving calls compose into engine-owned scratch and run an existing call against
 * those rows, request q standing where user q stood -- same kernels, same order, same score words as that call on an engine whose
 * Personal_Memory is the composed rows (with user_base 0 and the options "user_high_table" / "pm_bf16" off):
 *   m2d_topk_profiles          excl_off == NULL: m2d_topk_users (1 <= k <= min(64, I)); otherwise m2d_topk_users_excluding
 *                              (1 <= k <= min(16, I)), each with its own requirements, refusals and diagnostics;
 *   m2d_score_profiles         m2d_score_pairs_bydish over pairs (rows[b], items[b]), rows[b] a profile index: one outside [0, n) is
 *                              latched as M2D_ERR_BAD_USER_ID with its value and b;
 *   m2d_topk_markets_profiles  m2d_topk_markets_excluding, request q = (profile q, market q).
 * The engine's own Personal_Memory, shard base, derived tables and options are what they were when the call returns, on every path.
 * Returned directly as M2D_ERR_INVALID_ARG: a null batch, labels, general_memory or output, L < 1, n < 0 or n >= 2^31, an alpha that is
 * not finite.  n == 0: M2D_OK, nothing launched.  No call synchronises (beyond what the call it stands for does) or allocates after
 * its first launch of a size.  general_memory is read as it stands when the kernel runs on `stream`. */
typedef struct {
    const int32_t *users;            /* device i32[n] or NULL (all guests); -1 = guest */
    const float *labels;             /* device f32[n, L] */
    const float *general_memory;     /* device f32[L, C+1, E] */
    int64_t n;
    int32_t L;
    float alpha;
} m2d_profile_batch;

int m2d_compose_profiles(m2d_engine *h, const m2d_profile_batch *p, float *out_rows /* device, [n, C+1, E] */, void *stream);
int m2d_topk_profiles(m2d_engine *h, const m2d_profile_batch *p, int32_t k,
                      const int64_t *excl_off /* device, [n + 1], NULL = no exclusions */,
                      const int32_t *excl_ids /* device, [excl_off[n]] */, float *out_scores /* device, [n, k] */,
                      int32_t *out_ids /* device, [n, k] */, void *stream);
int m2d_score_profiles(m2d_engine *h, const m2d_profile_batch *p, const int32_t *rows /* device, [B]: profile index */,
                       const int32_t *items /* device, [B] */, int64_t B, float *out /* device, [B] */, void *stream);
int m2d_topk_markets_profiles(m2d_engine *h, const m2d_profile_batch *p, const int64_t *market_off /* device, [n + 1] */,
                              const int32_t *market_ids /* device, [nnzM], may be null when nnzM == 0 */, int64_t nnzM,
                              const int64_t *excl_off /* device, [n + 1], NULL = no exclusions */,
                              const int32_t *excl_ids /* device, [excl_off[n]] */, int32_t k, int32_t max_missing,
                              float *out_scores /* device, [n, k] */, int32_t *out_ids /* device, [n, k] */,
                              int32_t *out_counts /* device, [n], may be null */,
                              int32_t *out_missing /* device, [n, k, max_missing], may be null */, void *stream);

/* Synchronise `stream` and report (then clear) the first id error latched by kernels since the
 * previous check: M2D_OK, M2D_ERR_BAD_USER_ID or M2D_ERR_BAD_ITEM_ID.  TF-CPU GatherV2 raises
 * InvalidArgument for such ids; the kernels never read out of bounds and write NaN for the pair.
 * M2D_ERR_INVALID_ARG: an exclusion list of m2d_catalogue_rank / m2d_topk_users_excluding is not ascending (bad_value: the id or offset, bad_index: its
 * position in excl_ids / excl_off), or a slate entry of m2d_score_slate / m2d_topk_slate is not above its predecessor (bad_value: the id,
 * bad_index: its position in the slate), or a market segment of m2d_topk_markets decreases or reaches outside [0, nnzM] (bad_value: its
 * end offset, bad_index: the request).  M2D_ERR_BAD_INGREDIENT: a market id out of range (m2d_cookable_dishes, m2d_topk_markets).
 * bad_value / bad_index (host pointers, may be NULL) receive the offending id and its position.
 * m2d_topk_markets_excluding: its market and user errors are m2d_topk_markets'; an excluded id out of range is M2D_ERR_BAD_ITEM_ID
 * (bad_index: its position in excl_ids), an excluded id below its predecessor M2D_ERR_INVALID_ARG (the id, its position in excl_ids), an
 * exclusion segment that decreases or reaches outside the array M2D_ERR_INVALID_ARG (its end offset, that offset's index in excl_off). */
int m2d_check(m2d_engine *h, void *stream, int64_t *bad_value, int64_t *bad_index);

/* Options.  m2d_score_pairs* -- the reference path (Model_Recommender.py:56-97) -- is exact float32 whatever is set here, "pm_bf16"
 * excepted (exact float32 arithmetic on the bf16-rounded Personal_Memory).
 * Unknown names: M2D_ERR_INVALID_ARG.  "Results" = the scores / ids a call returns.
 *
 * ---- product switches -------------------------------------------------------------------------------------------------------------
 * name             default  values  changes results?                          what it does
 * skip_masked      1        0 / 1   no while every table value is finite      Pair kernels do not fetch the Personal_Memory row of a category whose
 *                                   (same bits); with inf / NaN in a table    mask weight is exactly 0 -- the graph multiplies it by 0 (:82) -- so a pair
 *                                   the engine ignores it and multiplies      moves (2 + active categories) E 4 B of rows, not (C + 2) E 4 B; a device word
 *                                   everything (the graph's NaNs)             "a table value is not finite" (table scan queued by m2d_create /
 *                                                                             m2d_tables_updated, the engine's writers on what they write) switches it
 *                                                                             off.  m2d_score_pairs_mlp: pairs grouped by the dish's pattern of non-zero
 *                                                                             weights, k-blocks a pattern lacks not multiplied.  0 = literal fetch-and-multiply.
 * user_high_table  0        0 / 1   scores within 1e-6 (another summation     Calls of >= 2^18 pairs read sum_c m_c <U_high[u], CE_c> / n from a derived
 *                                   order)                                    [U, 4] table (16 B per user; rebuilt after the engine's writers or
 *                                                                             m2d_tables_updated) instead of the U_high row.  A serving option.
 * pm_bf16          0        0 / 1   yes: the graph on the bf16-rounded        The C = 4 pair kernels (C = 4, E a multiple of 4 up to 256, "variant" != 9) read a
 *                                   Personal_Memory                           pair's Personal_Memory rows from a bf16 mirror of the table: (1 + active
 *                                                                             categories) E 2 B of user rows per pair instead of E 4 B each.  Any batch
 *                                                                             size; see "Serving mirror" below.
 * host_zero_copy   2        0 1 2   no                                        m2d_score_pairs_host up to 65 536 pairs: 2 = the kernel works on the pinned
 *                                                                             block and the call spins on a completion word, 1 = without the spin, 0 = staged copies.
 * topk_bf16x3      1        0 / 1   scores within ~1e-5 relative; dish ids    m2d_topk_users, 0/1 masks, E = 64 / 128: contraction on split-bf16 MFMA
 *                                   identical while topk_refine = 1           (x = hi + lo, three bf16 products, f32 accumulation).  0 = exact-f32 MFMA.
 * topk_refine      1        0 / 1   ids of near-tied lists (E = 32 / 64 /     Pattern-grouped kernels finish lists whose neighbouring scores -- or last
 *                                   128; k <= 10 at E = 128 split bf16)       entry and best score left out -- lie within twice the kernel's rounding
 *                                                                             margin in ONE plain-f32 arithmetic, so split-bf16 and exact-f32 return the
 *                                                                             same ids (a few per cent of the users re-scored; no measurable cost).
 *                                                                             0 = lists as the scan leaves them, ties at a list's end repaired.
 * topk_grouped     1        0 / 1   scores within the 1e-4 bar; both forms    0/1 masks, C = 4, k <= 16: dishes sorted by mask pattern, contraction over E
 *                                   resolve ties to the lower dish id         (m2d_topk_users above).  0 = the dense kernel over (C + 1) E (about 5x the work).
 * mlp_bf16x3       1        0 / 1   scores within ~1e-5 relative              Layers 1-2 of m2d_score_pairs_mlp on split-bf16 MFMA.  0 = exact-f32 MFMA.
 *
 * ---- diagnostic / A-B values: kernel selection for benchmarking and tests; results never depend on them (same bits) unless noted ------
 * name             default  values
 * prefetch         2        1 / 2 / 4    row-load steps issued ahead in the pair kernels
 * nt_loads         1        0 / 1        non-temporal loads of Personal_Memory rows
 * blocks_per_cu    8        1 ... 16     grid size of the pair kernels
 * mlp_form         0        0 / 1        split-bf16 head kernel: 0 = matrix waves fed by gather / DMA waves, 1 = every wave gathers its own rows
 *                                        (same results within the split's rounding)
 * topk_form        0        0 ... 4      split-bf16 retrieval kernel: 0 / 2 = pipelined form, 1 = first form (same lists).  Large catalogues (more than
 *                                        24 576 tiles of 32 dishes at E = 64, more than 10 240 at E = 128; with the ingredient table, where every tile
 *                                        is multiplied, more than 256): the pipelined form multiplies the hi x hi
 *                                        product of every tile and the two cross products only for tiles that can still hold a candidate -- scores
 *                                        are within the split's rounding of the three-product kernels' but not their bits, which is why the rule looks
 *                                        at the catalogue alone (blocks of 256 users; "topk_block" = 128 is not honoured there).  3 = that form for
 *                                        any catalogue, 4 = never (both diagnostic)
 * topk_prune       1        0 1 2 4 5 7 9  pattern-grouped retrieval: 1 = scan starts from a lower bound of the user's k-th score and steps through the
 *                                        tiles of the mask patterns that can reach its top-k only (bounds: alpha_P[u] +- |w_P[u]| max|RE[d]|, widened by
 *                                        what the arithmetic can move a computed score by; users sorted by pattern mask; (user block, dish range) items
 *                                        longest first); 0 = every tile.  A/B forms the tests compare with it: 2 the bound only, 4 the patterns only, 5 the
 *                                        grid's launch order, 7 a user's dish ranges keep their thresholds apart (by default they meet in one atomic-max
 *                                        word per user, E = 64), 9 the tie repair reads every pattern's dishes.  Same lists, bit for bit.
 * topk_block       0        0 128 256    users per block of a pruned pipelined launch (0 = the launcher's choice)
 * topk_excl_tier   0        0 / 2        m2d_topk_users_excluding: 0 = m2d_topk_users' lists filtered where they are index-exact, the exact scan
 *                                        for the users left short and for every other case; 2 = the exact scan for every user.  Same ids, same score bits.
 * market_shares    0        0 ... 64     m2d_topk_markets: shares of the catalogue per request: 0 = clamp(4 num_cu / nQ, 1, min(64, ceil(I / 256))),
 *                                        1 ... 64 forced (clamped to the catalogue's 256-dish blocks).  Same ids, same score bits, same counts.
 * topk_mlp_chunk_pairs  4194304  256 ... 2^24  m2d_topk_users_mlp: pairs per head launch (the --workload mlp batch by default); other values are
 *                                        M2D_ERR_INVALID_ARG.  Same ids, same score bits.
 * slate_chunk_pairs  4194304  256 ... 2^24  m2d_topk_slate: pairs of score scratch one pass may hold (user blocks of max(1, P / nD) rows); other values
 *                                        are M2D_ERR_INVALID_ARG.  Same ids, same score bits.
 * deep_chunk_pairs   4194304  256 ... 2^24  m2d_topk_users_deep (and stage 1 of m2d_topk_users_mlp_deep): dish ranges of W = min(I, P, 65536) dishes, user
 *                                        blocks of max(1, P / W) rows; other values are M2D_ERR_INVALID_ARG.  Same ids, same score bits.
 * menu_select      0        0 / 1        m2d_topk_menu, m2d_topk_menu_filtered: the selection behind each signature's candidate list: 0 = the list across a wave's lanes
 *                                        (m2d_topk_mlp_select), 1 = the radix select (m2d_select_deep).  Same ids, same score bits.
 * variant        0        7 9 11 12 13 14 15 16, 100 + n
 *                                        7 / 9: retrieval on the dense MFMA kernel / on the one-block-per-user kernel; 9 also forces the generic pair,
 *                                        head and slate kernels; 11 / 12: the pair kernel's throughput / latency form whatever the batch size; 13: tie
 *                                        repair's one-block-per-user tier from the third listed user on; 14: the nine-launch training step;
 *                                        15: the retrieval scan's progress-word wait gives up at once (M2D_ERR_KERNEL_TIMEOUT: test hook);
 *                                        16: the MLP head's row offsets in 16-byte units (the instantiation tables of 4 GiB and more take);
 *                                        100 + n: n dish-range splits in retrieval
 * (round 6 removed the values no test or profile script used: topk_prune 3 / 6, topk_probes, variant 8)
 *
 * ---- read-only diagnostics of the last m2d_topk_users call (m2d_get_option; they synchronise the device) ---------------------------------
 * topk_repaired          users the tie repair re-ranked over their patterns
 * topk_refined           users whose near-tied list m2d_topk_refine finished;  topk_refine_repaired: of those, sent on to the tie repair
 * topk_tiles_scanned     32-dish tiles the blocks stepped through;  topk_tiles_full: what they would have without pruning
 * topk_tiles_completed   the hi x hi first form (see topk_form): (wave, tile) pairs whose cross products were multiplied; -1 if another form ran
 * topk_block_users       users per block of that launch (128 or 256);  num_cu: compute units of the device
 *
 * ---- read-only diagnostics of the last m2d_catalogue_rank call (they synchronise the device) ------------------------------------------------
 * rank_tiles_scanned     32-dish tiles the count kernel multiplied (tiles whose bound settled every query of a wave are counted unmultiplied)
 * rank_resolved          (query, dish) pairs decided in the exact arithmetic
 *
 * ---- read-only diagnostics of the last m2d_topk_users_excluding call (they synchronise the device) ------------------------------------------
 * topk_excl_short          users sent to the exact scan: those the filter left with fewer than k dishes, or all of them
 * topk_excl_tiles_scanned  32-dish tiles the exact scan multiplied
 * (the "topk_*" diagnostics above then describe the call's internal m2d_topk_users retrieval, if its first tier ran)
 *
 * ---- read-only diagnostic of the last m2d_topk_markets call (host value, no synchronisation) -----------------------------------------------
 * market_shares_used       shares per request the launcher used
 *
 * ---- read-only diagnostic of the last m2d_topk_users_mlp call (host counter, no synchronisation) --------------------------------------------
 * topk_mlp_launches        head launches: user blocks x dish ranges (two-stage: user blocks; the "topk_*" diagnostics then describe stage 1)
 */
int m2d_set_option(m2d_engine *h, const char *name, int64_t value);
int m2d_get_option(const m2d_engine *h, const char *name, int64_t *value);

/* Calibration probe, not part of the scoring path: a plain 16-B-per-lane streaming read of `bytes`
 * bytes (multiple of 16) that folds everything into sink[0]; bench.py times it to report the
 * achievable HBM read rate of the box beside the 8 TB/s spec peak. */
int m2d_stream_read_probe(m2d_engine *h, const void *buf, int64_t bytes, float *sink, void *stream);

/* Name of the kernel the last m2d_score_pairs* call launched (for matching rocprofv3 traces). */
const char *m2d_last_kernel(const m2d_engine *h);

#ifdef __cplusplus
}
#endif
#endif /* M2D_H_ */
