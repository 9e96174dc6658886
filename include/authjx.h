/*
 * authjx.h — C-ABI of libauthjx.so, the MI355X-native batched evaluator for Authorino's
 * pattern-matching authorization hot path.
 *
 * Plain C types only (pointers, sizes, integers); no torch / HIP types in signatures
 * (`stream` is an opaque hipStream_t passed as void*).
 *
 * Concurrency: every function may be called from any thread. Compiled rulesets are
 * immutable after authjx_compile and may be shared by any number of threads and
 * contexts of their device (the reference shares expression trees across goroutines:
 * pkg/service/auth.go:300 copies AuthConfig by value, sharing its trees). A context
 * keeps one workspace (set table, capture rows, exact-scan list, request order) per
 * stream it is called with: batches on different streams of one context run
 * concurrently without sharing scratch; calls on one stream are serialised (their
 * kernels are ordered by the stream). authjx_free waits for the last batch of every
 * stream that used the ruleset, nothing else. The host-buffer entry points
 * (authjx_eval_batch, authjx_select_batch) use the context's own stream, one call at a
 * time. For many concurrent callers with one request each, use the micro-batcher
 * (authjx_batcher_*), which forms the batches.
 *
 * Interface each entry point replaces (reference = modassarrana89/authorino):
 *   authjx_compile          controllers/auth_config_controller.go:805-852
 *                           buildJSONExpression / buildJSONExpressionPattern(s): the
 *                           reconcile-time construction of a jsonexp tree. Here the tree
 *                           (flattened, see authjx_tree) is compiled once into
 *                           device-resident tables (selector paths, literal pool,
 *                           fold bytecode, regex DFAs).
 *   authjx_compile_forest   the same compile point for every expression of one
 *                           AuthConfig's authorization phase at once (one document scan
 *                           per request for all of them).
 *   authjx_free             pkg/auth/auth.go:30-33 AuthConfigCleaner.Clean (called from
 *                           pkg/evaluators/config.go:42-68 before re-translate/delete).
 *   authjx_eval_batch[_device]
 *                           pkg/jsonexp/expressions.go:102-104 Expression.Matches(json)
 *                           (Pattern.Matches :59-96, And :111-125, Or :136-154) for a
 *                           micro-batch of Authorization-JSON documents; its callers are
 *                           pkg/evaluators/authorization/json.go:19 (JSON rules) and
 *                           pkg/service/auth_pipeline.go:382 (every `when` gate).
 *   authjx_select_batch[_device]
 *                           pkg/json/json.go:41-53 JSONValue.ResolveFor's
 *                           gjson.Get(authJSON, pattern) (and the per-placeholder Get of
 *                           ReplaceJSONPlaceholders, :96-151) for a micro-batch: the
 *                           selector values behind response headers
 *                           (pkg/evaluators/response.go:150-174), returned as spans of
 *                           the document that the host formats (Value()/String()).
 *   authjx_pattern_error    the static error a pattern yields (regexp.Compile's
 *                           "error parsing regexp: ..." or expressions.go:94
 *                           "unsupported operator for json authorization").
 */
#ifndef AUTHJX_H
#define AUTHJX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AUTHJX_ABI_VERSION 1

/* return codes */
#define AUTHJX_OK 0
#define AUTHJX_EINVAL (-1)
#define AUTHJX_ENOMEM (-2)
#define AUTHJX_EDEVICE (-3)
#define AUTHJX_ELIMIT (-4)
#define AUTHJX_ETIMEDOUT (-5) /* micro-batcher: the deadline passed before evaluation */
#define AUTHJX_ECLOSED (-6)   /* micro-batcher: destroyed while the request waited for room */
#define AUTHJX_EEXIST (-7)    /* index: the key is taken and override was not asked for */

/* jsonexp.Operator (pkg/jsonexp/expressions.go:12-19) */
#define AUTHJX_OP_UNKNOWN 0
#define AUTHJX_OP_EQ 1
#define AUTHJX_OP_NEQ 2
#define AUTHJX_OP_INCL 3
#define AUTHJX_OP_EXCL 4
#define AUTHJX_OP_MATCHES 5

/* tree node kinds: jsonexp.Pattern, *jsonexp.And, *jsonexp.Or */
#define AUTHJX_NODE_PATTERN 0
#define AUTHJX_NODE_AND 1
#define AUTHJX_NODE_OR 2

/* Tri-state result of Expression.Matches: (false,nil)=F, (true,nil)=T, (false,err)=E.
 * UNDECIDED: the result depends on a pattern compiled as AUTHJX_PAT_UNSUPPORTED, or on
 * a hex mantissa / '_'-separated number literal (never valid JSON); the caller must not
 * take a decision from it and routes that request to its own evaluator. Every JSON
 * number is decided: Go ParseFloat + FormatFloat(f, 'f', -1, 64) run exactly on the
 * device (ajx_float.h). */
#define AUTHJX_F 0
#define AUTHJX_T 1
#define AUTHJX_E 2
#define AUTHJX_UNDECIDED 3

/* per-pattern compile status */
#define AUTHJX_PAT_OK 0
#define AUTHJX_PAT_STATIC_ERROR 1 /* Matches always returns (false, err): bad regex / op */
#define AUTHJX_PAT_UNSUPPORTED 2  /* selector / regex syntax not compiled for the device */

typedef struct authjx_ctx authjx_ctx;
typedef struct authjx_ruleset authjx_ruleset;

typedef struct {
    const char* selector; /* gjson path (jsonexp.Pattern.Selector) */
    uint32_t selector_len;
    int32_t op; /* AUTHJX_OP_* */
    const char* value; /* jsonexp.Pattern.Value */
    uint32_t value_len;
} authjx_pattern;

typedef struct {
    int32_t kind;  /* AUTHJX_NODE_* */
    int32_t left;  /* node index or -1 (nil) */
    int32_t right; /* node index or -1 (nil) */
    int32_t pattern; /* pattern index for AUTHJX_NODE_PATTERN */
} authjx_node;

/* One jsonexp.Expression, flattened. root = -1 means a nil Expression. */
typedef struct {
    const authjx_pattern* patterns;
    uint32_t n_patterns;
    const authjx_node* nodes;
    uint32_t n_nodes;
    int32_t root;
} authjx_tree;

/* Device context: one per GPU (device ordinal). authjx_shutdown first destroys every
 * micro-batcher still alive on the context (authjx_batcher_destroy: queued requests are
 * evaluated); their handles are invalid afterwards. */
int authjx_init(int device, authjx_ctx** out);
void authjx_shutdown(authjx_ctx* ctx);
/* Release the per-stream workspace (capture rows, slow list, order, set table) the
 * context keeps for `stream` since its first device call on it: for callers that use
 * short-lived streams. Not the context's own stream. The workspace is reference-counted:
 * a call still running on that stream, or an authjx_last_* reader, keeps it until that
 * call returns, and whichever thread drops the last reference (this one, or that call's)
 * waits for the stream's last batch before freeing it, so this call may return before
 * that batch has ended. Only authjx_shutdown must not race the context's calls. */
int authjx_release_stream(authjx_ctx* ctx, void* stream);
// The sha256 (first 32 hex digits) of the sources the library was built from
// (authorino_amd/build.py source_hash); the Python runtime refuses a stale binary.
const char* authjx_build_hash(void);
int authjx_device_count(void);

/* Compile one tree into a device-resident ruleset. pattern_status (n_patterns entries,
 * may be NULL) receives AUTHJX_PAT_*. A ruleset that contains UNSUPPORTED patterns is
 * still created; evaluating it yields AUTHJX_UNDECIDED for requests whose result
 * depends on them. errbuf (may be NULL) receives a diagnostic. */
int authjx_compile(authjx_ctx* ctx, const authjx_tree* tree, authjx_ruleset** out,
                   int32_t* pattern_status, char* errbuf, size_t errcap);
/* Compile several trees that read the same documents into ONE ruleset, so that one
 * scan of a document evaluates all of them (an authorization phase: the AuthConfig-level
 * `when`, each evaluator's `when` and rules — pkg/service/auth_pipeline.go:120-125,
 * :287-322, :454-457). Patterns are numbered across the trees in order (tree k's
 * pattern i is pattern sum_{j<k} n_patterns_j + i; pattern_status has that many
 * entries); selectors shared by several trees are scanned once. Evaluating it writes
 * one result per tree: d_out_tristate[r * n_trees + k] and d_out_err_idx[r * n_trees + k]
 * (the error index in the forest's numbering). Every ruleset of one batch must have the
 * same tree count. */
int authjx_compile_forest(authjx_ctx* ctx, const authjx_tree* trees, uint32_t n_trees, authjx_ruleset** out,
                          int32_t* pattern_status, char* errbuf, size_t errcap);
/* Results per request of the ruleset (1 for authjx_compile). */
uint32_t authjx_ruleset_trees(const authjx_ruleset* rs);
void authjx_free(authjx_ruleset* rs);
uint32_t authjx_ruleset_patterns(const authjx_ruleset* rs);
uint32_t authjx_ruleset_selectors(const authjx_ruleset* rs);
/* Copies the static error text of pattern i ("" when it has none); returns its length. */
size_t authjx_pattern_error(const authjx_ruleset* rs, uint32_t i, char* buf, size_t cap);

/* Evaluate a batch whose documents are already in device memory (HBM).
 *   sets[n_sets]      rulesets; request r uses sets[set_of_req ? set_of_req[r] : 0]
 *   d_set_of_req      device u32[n] (entries < n_sets) or NULL; ignored when n_sets == 1
 *   d_arena           device bytes; document r = d_arena[d_offs[r] .. + d_lens[r]). The
 *                     kernels read whole aligned 32-byte blocks (the streaming kernel's
 *                     unit; the others read 16): every block holding a document byte must
 *                     be readable (device allocations are; an arena carved from a larger
 *                     buffer needs 31 readable bytes after its end)
 *   d_out_tristate    device u8[n * n_trees]  (AUTHJX_F/T/E/UNDECIDED; n_trees = 1 unless
 *                     the rulesets come from authjx_compile_forest)
 *   d_out_err_idx     device i32[n * n_trees] pattern whose error decided an E, else -1
 *                     (may be NULL)
 *   d_out_bitmap      device u64[n * bitmap_stride_words]: bit p = pattern p evaluated to T
 *                     (every pattern evaluated, no short-circuit), may be NULL
 *   stream            hipStream_t (NULL = the context's stream). Asynchronous. */
int authjx_eval_batch_device(authjx_ctx* ctx, const authjx_ruleset* const* sets, uint32_t n_sets,
                             const uint32_t* d_set_of_req, const uint8_t* d_arena,
                             const uint64_t* d_offs, const uint32_t* d_lens, uint32_t n,
                             uint8_t* d_out_tristate, int32_t* d_out_err_idx,
                             uint64_t* d_out_bitmap, uint32_t bitmap_stride_words, void* stream);

/* Same, from host buffers: copies to the device, evaluates, copies back; synchronous.
 * This is the entry point a cgo shim's micro-batcher calls. */
int authjx_eval_batch(authjx_ctx* ctx, const authjx_ruleset* const* sets, uint32_t n_sets,
                      const uint32_t* set_of_req, const uint8_t* arena, uint64_t arena_len,
                      const uint64_t* offs, const uint32_t* lens, uint32_t n,
                      uint8_t* out_tristate, int32_t* out_err_idx, uint64_t* out_bitmap,
                      uint32_t bitmap_stride_words);

/* gjson.Get(doc, selector) as a span of the document. type is gjson.Type
 * (AUTHJX_JSON_*); start is relative to the document; for strings the span includes the
 * quotes and esc = 1 when the contents hold a backslash escape. A missing path is
 * {0, 0, AUTHJX_JSON_NULL}. AUTHJX_JSON_UNSUPPORTED: the selector uses gjson syntax the
 * device does not compile (its pattern_status is AUTHJX_PAT_UNSUPPORTED). */
#define AUTHJX_JSON_NULL 0
#define AUTHJX_JSON_FALSE 1
#define AUTHJX_JSON_NUMBER 2
#define AUTHJX_JSON_STRING 3
#define AUTHJX_JSON_TRUE 4
#define AUTHJX_JSON_JSON 5
#define AUTHJX_JSON_UNSUPPORTED 255
#define AUTHJX_VALUE_COUNT 2 /* authjx_value.esc: `start` is an array's element count (a
                              * last path part "#", gjson parseArray), len 0: no span */
#define AUTHJX_VALUE_TEXT 4  /* authjx_value.esc flag (with 1 = escapes): the value is built
                              * text — the Result of a modifier chain or a "#." list — at
                              * [start, start + len) of the request's text slot
                              * (authjx_select_text_batch[_device]) */
typedef struct {
    uint32_t start;
    uint32_t len;
    uint8_t type;
    uint8_t esc; /* 1: a string with escapes (gjson unescape applies); AUTHJX_VALUE_COUNT */
    uint16_t reserved;
} authjx_value;

/* Resolve the selector of every pattern of `sets[set_of_req[r]]` (operators and values
 * are ignored; compile the selectors as a tree of AUTHJX_OP_EQ patterns with root -1)
 * for every request: d_out_values[r * values_stride + p], values_stride >= the largest
 * n_patterns. Device buffers, asynchronous on `stream` (NULL = the context's stream). */
int authjx_select_batch_device(authjx_ctx* ctx, const authjx_ruleset* const* sets, uint32_t n_sets,
                               const uint32_t* d_set_of_req, const uint8_t* d_arena, const uint64_t* d_offs,
                               const uint32_t* d_lens, uint32_t n, authjx_value* d_out_values,
                               uint32_t values_stride, void* stream);
/* The values of patterns [first_pattern, first_pattern + values_stride) of `rs` from the
 * capture rows the last authjx_eval_batch_device call on this context wrote: that call
 * must have evaluated `rs` alone over the same d_arena / d_offs / d_lens (n requests),
 * without authjx_set_exact_scan, and `rs` must come from authjx_compile_forest (the
 * default kernel keeps capture rows for forests only). For a phase compiled with authjx_compile_forest whose
 * last tree holds the response selectors (AUTHJX_OP_EQ patterns, root -1), this resolves
 * them without a second document scan: the gjson.Get of JSONValue.ResolveFor
 * (pkg/json/json.go:41-53) after the rules of the same request. The patterns must belong
 * to root-less trees of the forest (the kernel writes capture records only for those and
 * for the values its stage B reads). AUTHJX_EINVAL when the rows are not that
 * evaluation's, or a pattern's record is not kept. Asynchronous on `stream`; order it
 * after the eval. */
int authjx_select_from_eval_device(authjx_ctx* ctx, const authjx_ruleset* rs, uint32_t first_pattern,
                                   const uint8_t* d_arena, const uint64_t* d_offs, const uint32_t* d_lens,
                                   uint32_t n, authjx_value* d_out_values, uint32_t values_stride, void* stream);
/* Same from host buffers; synchronous. */
int authjx_select_batch(authjx_ctx* ctx, const authjx_ruleset* const* sets, uint32_t n_sets,
                        const uint32_t* set_of_req, const uint8_t* arena, uint64_t arena_len,
                        const uint64_t* offs, const uint32_t* lens, uint32_t n, authjx_value* out_values,
                        uint32_t values_stride);
/* authjx_select_batch[_device] for selectors with gjson modifiers (`a.b|@case:upper`,
 * `@extract:{...}`, ...) and "#." lists: their values are built text, not document spans
 * — the response / denyWith / cache-key templates of pkg/json/json.go:96-151 and
 * pkg/evaluators/authorization.go:56-66. Request r's text slot is
 * out_text[r * text_stride, (r + 1) * text_stride); a value esc has AUTHJX_VALUE_TEXT and
 * start / len within that slot. A value that does not fit, or that the device leaves
 * undecided (@case / @strip on a code point its Unicode tables do not vouch for), is
 * AUTHJX_JSON_UNSUPPORTED. Plain selectors are document spans as above. */
int authjx_select_text_batch_device(authjx_ctx* ctx, const authjx_ruleset* const* sets, uint32_t n_sets,
                                    const uint32_t* d_set_of_req, const uint8_t* d_arena, const uint64_t* d_offs,
                                    const uint32_t* d_lens, uint32_t n, authjx_value* d_out_values,
                                    uint32_t values_stride, uint8_t* d_out_text, uint32_t text_stride, void* stream);
int authjx_select_text_batch(authjx_ctx* ctx, const authjx_ruleset* const* sets, uint32_t n_sets,
                             const uint32_t* set_of_req, const uint8_t* arena, uint64_t arena_len,
                             const uint64_t* offs, const uint32_t* lens, uint32_t n, authjx_value* out_values,
                             uint32_t values_stride, uint8_t* out_text, uint32_t text_stride);

/* Route every request through the exact per-selector scan kernel instead of the
 * single-pass kernel (results are identical; used to cross-check the two paths). */
int authjx_set_exact_scan(authjx_ctx* ctx, int force);
/* Number of requests of the last batch the single-pass kernel handed to the exact scan
 * (documents it could not prove gjson-equivalent, e.g. not valid JSON). Synchronises. */
int64_t authjx_last_exact_count(authjx_ctx* ctx);

/* Kernel-only timing of the last device call on the context (its stream's events
 * around the launches, ms). */
float authjx_last_kernel_ms(authjx_ctx* ctx);

/* ---- micro-batcher --------------------------------------------------------------
 * Replaces the per-request evaluation made from each request's own goroutine
 * (pkg/service/auth_pipeline.go:150-164 evaluator goroutines; main.go:69,451 up to 10k
 * concurrent streams): callers submit one request each and block; a worker thread
 * flushes a batch when max_batch requests are queued or the oldest has waited
 * window_us, drops requests whose deadline passed (AUTHJX_ETIMEDOUT, not evaluated),
 * orders the rest by ruleset (AuthConfig buckets) and evaluates them with one launch on
 * the batcher's own stream (rulesets of one batch share n_trees; others wait for the
 * next batch). The queue holds at most queue_cap requests (0: 4 * max_batch); a caller
 * waits for room up to its deadline. */
typedef struct authjx_batcher authjx_batcher;
int authjx_batcher_create(authjx_ctx* ctx, uint32_t max_batch, uint32_t window_us, uint32_t queue_cap,
                          authjx_batcher** out);
/* Evaluates what is queued, then stops the worker (callers still waiting for room get
 * AUTHJX_ECLOSED). */
void authjx_batcher_destroy(authjx_batcher* b);
/* Blocking: Expression.Matches of `rs` on one document (copied at batch time; the
 * buffer must stay valid until return). timeout_us: 0 = no deadline. out_tristate /
 * out_err_idx (may be NULL): n_trees entries, as authjx_eval_batch writes them. */
int authjx_batcher_eval(authjx_batcher* b, const authjx_ruleset* rs, const uint8_t* doc, size_t len,
                        uint64_t timeout_us, uint8_t* out_tristate, int32_t* out_err_idx);
int authjx_batcher_stats(authjx_batcher* b, uint64_t* batches, uint64_t* requests, uint64_t* expired,
                         uint64_t* max_batch_seen);

/* ---- AuthConfig index (host) ----------------------------------------------------
 * pkg/index/index.go's authConfigTree (:37-243), native, for the micro-batcher's
 * per-request AuthConfig selection (config C4). Keys are hostnames ('*' labels are
 * wildcards); entries are ruleset ids (the `set_of_req` values of authjx_eval_batch).
 * Set = index.go:67-80 (AUTHJX_EEXIST: "authconfig already exists in the index" when the
 * key is taken and override is 0); DeleteKey = :93-98 (the key's entry is removed only
 * when it is this id's). Lookups take a shared lock, Set/DeleteKey an exclusive one
 * (the reference's RWMutex, :51). */
typedef struct authjx_index authjx_index;
int authjx_index_new(authjx_index** out);
void authjx_index_free(authjx_index* ix);
int authjx_index_set(authjx_index* ix, const char* key, uint32_t key_len, int32_t set_id, int override_);
int authjx_index_delete_key(authjx_index* ix, const char* key, uint32_t key_len, int32_t set_id);
/* Index.Get (index.go:56-65) with the ':port' retry of pkg/service/auth.go:270-280:
 * *out_set = the host's ruleset id, -1 when none (the reference answers NOT_FOUND,
 * auth.go:282-287). */
int authjx_index_get(const authjx_index* ix, const char* host, uint32_t host_len, int32_t* out_set);
/* The same for a micro-batch of hosts (host r = hosts[offs[r] .. offs[r] + lens[r])) on
 * n_threads host threads (0: all cores), each distinct host walked once per thread. */
int authjx_index_lookup_batch(const authjx_index* ix, const uint8_t* hosts, const uint64_t* offs,
                              const uint32_t* lens, uint32_t n, int32_t* out_sets, uint32_t n_threads);

/* ---- Authorization JSON packing (host) -------------------------------------------
 * The producer's output stage (pkg/service/auth_pipeline.go:542-616 GetAuthorizationJSON,
 * json.Marshal per evaluator call in the reference): each request's values, walked once
 * by the caller into a TAPE, are encoded with encoding/json's rules (HTML-safe string
 * escapes, U+2028/U+2029, invalid UTF-8 as \ufffd, map keys sorted by bytes, float64 'f'
 * or 'e' by magnitude) straight into the batch arena that authjx_eval_batch reads.
 * Tape (little-endian), one value:
 *   AUTHJX_TAPE_NULL / TRUE / FALSE
 *   AUTHJX_TAPE_F64 <8 B double>      float64 (NaN / Inf: the request fails, as Marshal does)
 *   AUTHJX_TAPE_I64 <8 B int64>       integer types
 *   AUTHJX_TAPE_STRING <u32 len><bytes>
 *   AUTHJX_TAPE_RAW <u32 len><bytes>  pre-encoded JSON (json.RawMessage), copied
 *   AUTHJX_TAPE_ARRAY <u32 n><n values>
 *   AUTHJX_TAPE_OBJECT <u32 n><n x (<u32 len><key bytes> value)>  a struct: member order kept
 *   AUTHJX_TAPE_MAP <u32 n><same>     a map: members written sorted by key bytes */
#define AUTHJX_TAPE_NULL 1
#define AUTHJX_TAPE_TRUE 2
#define AUTHJX_TAPE_FALSE 3
#define AUTHJX_TAPE_F64 4
#define AUTHJX_TAPE_I64 5
#define AUTHJX_TAPE_STRING 6
#define AUTHJX_TAPE_RAW 7
#define AUTHJX_TAPE_ARRAY 8
#define AUTHJX_TAPE_OBJECT 9
#define AUTHJX_TAPE_MAP 10
/* Request r's tape is tapes[tape_offs[r] .. + tape_lens[r]); its document goes to
 * arena[out_offs[r] .. + out_lens[r]), the documents back to back in request order, on
 * n_threads host threads (0: all cores). *out_total = the bytes the batch needs:
 * AUTHJX_ELIMIT (nothing written) when that exceeds arena_cap; AUTHJX_EINVAL when a
 * tape is malformed or holds a NaN / Inf (that request: out_offs = ~0, out_lens = 0). */
int authjx_pack_json(const uint8_t* tapes, const uint64_t* tape_offs, const uint32_t* tape_lens, uint32_t n,
                     uint8_t* arena, uint64_t arena_cap, uint64_t* out_offs, uint32_t* out_lens,
                     uint64_t* out_total, uint32_t n_threads);

/* Response header values rendered on the device. The select entry points return spans; a
 * render program, compiled once per AuthConfig, turns them into the bytes Authorino puts on
 * the wire: a Plain header (fmt.Sprintf("%v", gjson Value())), a template
 * (ReplaceJSONPlaceholders, pkg/json/json.go:96-151) or a DynamicJSON header (json.Marshal
 * of a map, then StringifyJSON). A program is a list of outputs (one per header), each a
 * list of ops over value slots: indices into the authjx_value[n][values_stride] array a
 * select call wrote (source bytes: the document, or the request's text slot when esc has
 * AUTHJX_VALUE_TEXT). Ops append:
 *   AUTHJX_R_LIT         lit[0, lit_len): template text, pre-rendered statics, {"name": scaffolding
 *   AUTHJX_R_STRING      gjson Result.String() of the value (a template placeholder)
 *   AUTHJX_R_STRING_ESC  the same bytes with encoding/json's string escaping, no quotes (a
 *                        template that is a DynamicJSON property value)
 *   AUTHJX_R_SPRINT      fmt.Sprintf("%v", Result.Value()): numbers through float64 and %g
 *                        (1685557675 -> 1.685557675e+09), nil "<nil>", arrays "[a b]", objects
 *                        "map[k:v k:v]" with keys sorted by bytes, the last duplicate kept
 *   AUTHJX_R_MARSHAL     json.Marshal(Result.Value()): HTML-safe string escapes, float64
 *                        numbers ('e' form below 1e-6 and from 1e21), sorted object keys. A
 *                        NaN / Inf under it makes Marshal fail: the whole output is empty,
 *                        status AUTHJX_RENDER_OK (StringifyJSON's error is dropped)
 * Each output of each request has a status. AUTHJX_RENDER_UNRENDERED: the caller renders
 * that header itself; the output appended nothing and the request's other outputs are not
 * disturbed. The reasons: a slot value of type AUTHJX_JSON_UNSUPPORTED; a number the device
 * leaves undecided (a hex mantissa or a '_' separator); containers nested deeper than 8
 * levels under SPRINT / MARSHAL; bytes that are not UTF-8 under STRING_ESC or MARSHAL's
 * string encoding; the output does not fit what is left of the request's output slot. */
#define AUTHJX_R_LIT 0
#define AUTHJX_R_STRING 1
#define AUTHJX_R_STRING_ESC 2
#define AUTHJX_R_SPRINT 3
#define AUTHJX_R_MARSHAL 4
/*   AUTHJX_R_STRINGIFY   json.StringifyJSON(Result.Value()) (pkg/json/json.go:153-159), a
 *                        denyWith message / body / header: a string's Result.String() bytes; a
 *                        number as FormatFloat(ParseFloat(raw), 'f', -1, 64) whatever its
 *                        spelling (12345678901234567890123 -> 12345678901234568000000, +-Inf:
 *                        the output is empty, status OK); true / false; null: nothing; an
 *                        object / array as MARSHAL writes it. Declines as MARSHAL does
 *   AUTHJX_R_STRING_UTF8 STRING that declines when the value's bytes are not UTF-8 (a
 *                        template placeholder under StringifyJSON, where Go writes U+FFFD) */
/* (op 5 is not assigned: authjx_render_compile answers AUTHJX_EINVAL for it, as before the
 * two ops above existed) */
#define AUTHJX_R_STRINGIFY 6
#define AUTHJX_R_STRING_UTF8 7
#define AUTHJX_RENDER_OK 0
#define AUTHJX_RENDER_UNRENDERED 1
/* the output does not apply under the request's verdict (the gated calls below): nothing
 * appended, none of its values read; its record is {write position, 0, SKIPPED} */
#define AUTHJX_RENDER_SKIPPED 2
typedef struct authjx_render authjx_render;
typedef struct {
    uint8_t op;         /* AUTHJX_R_* */
    uint32_t slot;      /* value slot (every op but LIT) */
    const uint8_t* lit; /* LIT: the bytes (copied by the compile) */
    uint32_t lit_len;
} authjx_render_op;
typedef struct {
    const authjx_render_op* ops;
    uint32_t n_ops;
} authjx_render_output;
typedef struct {
    uint32_t start, len; /* within the request's output slot */
    uint8_t status;      /* AUTHJX_RENDER_* */
    uint8_t reserved[3];
} authjx_rendered;
/* AUTHJX_EINVAL (and a message in errbuf) for an unknown op or a slot >= n_slots. */
int authjx_render_compile(authjx_ctx* ctx, const authjx_render_output* outs, uint32_t n_outputs, uint32_t n_slots,
                          authjx_render** out, char* errbuf, size_t errcap);
void authjx_render_free(authjx_render* prog);
uint32_t authjx_render_outputs(const authjx_render* prog);
/* Device buffers, asynchronous on `stream` (NULL: the context's stream); order it after
 * the select call that wrote d_values. d_text may be NULL when no value has
 * AUTHJX_VALUE_TEXT. d_out[r * n_outputs + k] is output k of request r, its bytes at
 * d_out_text[r * out_stride + start ...]; a request's outputs follow each other in its
 * slot, and the slot's bytes past the last output are unspecified. Nothing outside
 * [r * out_stride, (r + 1) * out_stride) is read or written. AUTHJX_EINVAL when
 * values_stride is below the program's n_slots, out_stride is 0 or no multiple of 16, or
 * d_out_text is not 16-byte aligned. */
int authjx_render_batch_device(authjx_ctx* ctx, const authjx_render* prog, const uint8_t* d_arena,
                               const uint64_t* d_offs, const uint32_t* d_lens, uint32_t n,
                               const authjx_value* d_values, uint32_t values_stride, const uint8_t* d_text,
                               uint32_t text_stride, uint8_t* d_out_text, uint32_t out_stride,
                               authjx_rendered* d_out, void* stream);
/* Same from host buffers (out_text needs no alignment); synchronous. */
int authjx_render_batch(authjx_ctx* ctx, const authjx_render* prog, const uint8_t* arena, uint64_t arena_len,
                        const uint64_t* offs, const uint32_t* lens, uint32_t n, const authjx_value* values,
                        uint32_t values_stride, const uint8_t* text, uint32_t text_stride, uint8_t* out_text,
                        uint32_t out_stride, authjx_rendered* out);

/* authjx_render_batch_device for a batch of several AuthConfigs: request r renders
 * progs[d_prog_of_req[r]] (device u32[n]; may be NULL when n_progs is 1: every request
 * renders progs[0]). AUTHJX_RENDER_NO_PROGRAM, or any entry
 * that is not below n_progs: the request reads nothing and writes nothing, neither its
 * output slot nor its records. Output k of request r is d_out[r * records_stride + k]
 * (records_stride >= the largest n_outputs; a program's records beyond its own n_outputs
 * are not written), its values d_values[r * values_stride ...] (values_stride >= the
 * largest n_slots). The table of program pointers is uploaded on `stream`. The checks of
 * authjx_render_batch_device, and AUTHJX_EINVAL as well when values_stride or
 * records_stride is below what a program needs, a program is NULL or of another device, or
 * n_progs > 1 and d_prog_of_req is NULL. */
#define AUTHJX_RENDER_NO_PROGRAM 0xFFFFFFFFu
int authjx_render_batch_multi_device(authjx_ctx* ctx, const authjx_render* const* progs, uint32_t n_progs,
                                     const uint32_t* d_prog_of_req, const uint8_t* d_arena, const uint64_t* d_offs,
                                     const uint32_t* d_lens, uint32_t n, const authjx_value* d_values,
                                     uint32_t values_stride, const uint8_t* d_text, uint32_t text_stride,
                                     uint8_t* d_out_text, uint32_t out_stride, authjx_rendered* d_out,
                                     uint32_t records_stride, void* stream);

/* ---- gated render: the verdict folded on the device, outputs chosen by it ------------
 * The fold of auth_pipeline.go's `when` gates and authorization phase over a request's
 * tri-states t[0, n_trees) (an authjx_compile_forest evaluation: one entry per expression):
 *   1. t[top_when_tree] UNDECIDED: the verdict is UNDECIDED; else not T: SKIPPED.
 *   2. The evaluators by priority level (runs of equal priority, in list order). A level
 *      that names an UNDECIDED tree (a `when` or rules, also the rules of an evaluator whose
 *      `when` is not met): UNDECIDED. Else its first evaluator whose `when` is absent or T
 *      and whose rules exist and are not T: DENIED, denied_by = its index; the fold stops.
 *   3. No level denies: GRANTED.
 * denied_by is -1 unless the verdict is DENIED. Output k of the render program then
 *   ALWAYS   renders;
 *   GRANTED  renders when the verdict is GRANTED and its when_tree is absent or T; is
 *            AUTHJX_RENDER_UNRENDERED when the verdict is GRANTED and that tree UNDECIDED;
 *   DENIED   renders when the verdict is DENIED;
 * under an UNDECIDED verdict every output but ALWAYS is AUTHJX_RENDER_UNRENDERED (the
 * caller's own evaluator decides such a request); every other output is
 * AUTHJX_RENDER_SKIPPED. A tree index of -1 stands for "none". */
#define AUTHJX_V_SKIPPED 0 /* the AuthConfig's `when` is not met: OK, no outputs */
#define AUTHJX_V_GRANTED 1
#define AUTHJX_V_DENIED 2
#define AUTHJX_V_UNDECIDED 3
typedef struct {
    int32_t when_tree, rules_tree, priority;
} authjx_gate_evaluator;
#define AUTHJX_GATE_ALWAYS 0
#define AUTHJX_GATE_GRANTED 1
#define AUTHJX_GATE_DENIED 2
typedef struct {
    uint8_t on; /* AUTHJX_GATE_* */
    int32_t when_tree;
} authjx_gate_output;
typedef struct {
    uint8_t verdict; /* AUTHJX_V_* */
    uint8_t reserved[3];
    int32_t denied_by;
} authjx_verdict;
typedef struct authjx_gates authjx_gates;
/* AUTHJX_EINVAL (and a message in errbuf): a tree index >= n_trees or below -1, priorities
 * that are not non-decreasing, an ALWAYS output with a when_tree, an unknown `on`. */
int authjx_gates_compile(authjx_ctx* ctx, int32_t top_when_tree, const authjx_gate_evaluator* evaluators,
                         uint32_t n_evaluators, const authjx_gate_output* outputs, uint32_t n_outputs,
                         uint32_t n_trees, authjx_gates** out, char* errbuf, size_t errcap);
void authjx_gates_free(authjx_gates* gates);
/* The same fold on the host (the function the kernel runs): tristate[0, n_trees), n_trees at
 * least the gates' own. */
int authjx_verdict_of(const authjx_gates* gates, const uint8_t* tristate, uint32_t n_trees, authjx_verdict* out);
/* authjx_render_batch_multi_device under gates: request r renders progs[d_prog_of_req[r]]
 * under gates[d_prog_of_req[r]] (a NULL entry: every output renders, no verdict is
 * written), folding d_tristate[(d_tri_of_req ? d_tri_of_req[r] : r) * tri_stride ...], where
 * an evaluation on the same stream left it. An output that does not apply is decided before
 * its first value is read. d_out_verdict (may be NULL): one authjx_verdict per request that
 * has a program and gates. The checks of the multi call, and AUTHJX_EINVAL as well for a
 * gates object whose n_outputs differs from its program's, whose n_trees exceeds tri_stride
 * or of another device, and for a NULL d_tristate when any gates entry is not NULL. */
int authjx_render_batch_gated_device(authjx_ctx* ctx, const authjx_render* const* progs, uint32_t n_progs,
                                     const uint32_t* d_prog_of_req, const uint8_t* d_arena, const uint64_t* d_offs,
                                     const uint32_t* d_lens, uint32_t n, const authjx_value* d_values,
                                     uint32_t values_stride, const uint8_t* d_text, uint32_t text_stride,
                                     uint8_t* d_out_text, uint32_t out_stride, authjx_rendered* d_out,
                                     uint32_t records_stride, const authjx_gates* const* gates,
                                     const uint8_t* d_tristate, uint32_t tri_stride, const uint32_t* d_tri_of_req,
                                     authjx_verdict* d_out_verdict, void* stream);
/* Same from host buffers (prog_of_req, tristate and tri_of_req too; tristate holds n rows,
 * or one more than the largest tri_of_req entry); synchronous. out / out_verdict entries
 * the kernel does not write keep the caller's bytes. */
int authjx_render_batch_gated(authjx_ctx* ctx, const authjx_render* const* progs, uint32_t n_progs,
                              const uint32_t* prog_of_req, const uint8_t* arena, uint64_t arena_len,
                              const uint64_t* offs, const uint32_t* lens, uint32_t n, const authjx_value* values,
                              uint32_t values_stride, const uint8_t* text, uint32_t text_stride, uint8_t* out_text,
                              uint32_t out_stride, authjx_rendered* out, uint32_t records_stride,
                              const authjx_gates* const* gates, const uint8_t* tristate, uint32_t tri_stride,
                              const uint32_t* tri_of_req, authjx_verdict* out_verdict);

/* ---- micro-batcher: a phase's response outputs with each decision -------------------
 * One AuthConfig as the serving path sees it: `rules` (authjx_compile or _forest: what
 * authjx_batcher_eval takes), `selectors` (authjx_compile, patterns {path, EQ, ""}, root -1:
 * slot k = pattern k) and the render program over those slots. Borrowed, not owned: free the
 * phase before any of the three. text_stride: bytes of built text per request (modifier
 * chains, "#." lists); 0: such values come back AUTHJX_JSON_UNSUPPORTED and their outputs
 * AUTHJX_RENDER_UNRENDERED, as after authjx_select_batch. out_stride: bytes of rendered
 * text per request. AUTHJX_EINVAL: a NULL argument; `selectors` has more than one tree, no
 * pattern, or fewer patterns than `prog` has slots; out_stride is 0 or no multiple of 16; the objects'
 * devices differ. AUTHJX_ELIMIT: out_stride or text_stride above 65536 (pinned staging per
 * request). */
typedef struct authjx_phase authjx_phase;
int authjx_phase_create(authjx_ctx* ctx, const authjx_ruleset* rules, const authjx_ruleset* selectors,
                        const authjx_render* prog, uint32_t text_stride, uint32_t out_stride, authjx_phase** out);
void authjx_phase_free(authjx_phase* ph);
uint32_t authjx_phase_outputs(const authjx_phase* ph);
/* Blocking, like authjx_batcher_eval, and batched with its requests: the decision (n_trees
 * entries) and, rendered from the same staged copy of the document in the same batch on the
 * same stream, every output of the program, whatever the decision (which outputs apply —
 * response headers after a grant, denyWith after a denial — is the caller's fold):
 * out[k] = {start, len, status} into out_text[0, out_stride), authjx_phase_outputs(ph)
 * records. out_text is written up to the end of the last output; its bytes past that, and
 * both buffers when the call does not return AUTHJX_OK (AUTHJX_ETIMEDOUT, a failed batch),
 * are left as they were. Requests of phases with different strides share a batch but not
 * a select / render launch.
 * Lifetime: the call returns after its batch's worker has synchronized the stream, so no
 * kernel reads a phase's ruleset, selectors or program once the last call on that phase
 * has returned; authjx_free / authjx_render_free then wait as they always do, and
 * authjx_shutdown destroys the batchers first. */
int authjx_batcher_phase(authjx_batcher* b, const authjx_phase* ph, const uint8_t* doc, size_t len,
                         uint64_t timeout_us, uint8_t* out_tristate, int32_t* out_err_idx,
                         uint8_t* out_text, authjx_rendered* out);

/* A phase under gates (authjx_gates_compile over the trees of `rules`): its requests take
 * the gated render, so only the outputs that apply under the request's verdict are rendered
 * (the others AUTHJX_RENDER_SKIPPED, no bytes) and the verdict comes back with them. The
 * batch's tri-states are read where the evaluation left them in device memory. A batch that
 * mixes gated and ungated phases takes one gated launch per stride group (an ungated
 * phase's requests render every output, as before). `gates` is borrowed like the other
 * three. AUTHJX_EINVAL: authjx_phase_create's cases; gates whose n_outputs differs from the
 * program's, whose n_trees exceeds the rules' trees, or of another device. */
int authjx_phase_create_gated(authjx_ctx* ctx, const authjx_ruleset* rules, const authjx_ruleset* selectors,
                              const authjx_render* prog, const authjx_gates* gates, uint32_t text_stride,
                              uint32_t out_stride, authjx_phase** out);
/* authjx_batcher_phase on a gated phase, with the verdict (out_verdict may be NULL).
 * AUTHJX_EINVAL for an ungated phase. authjx_batcher_phase itself also accepts a gated
 * phase (the same outputs, no verdict) and is unchanged for an ungated one. */
int authjx_batcher_phase_gated(authjx_batcher* b, const authjx_phase* ph, const uint8_t* doc, size_t len,
                               uint64_t timeout_us, uint8_t* out_tristate, int32_t* out_err_idx,
                               uint8_t* out_text, authjx_rendered* out, authjx_verdict* out_verdict);

#ifdef __cplusplus
}
#endif
#endif
