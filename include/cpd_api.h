/*
 * cpd_api.h — C ABI of the MI355X-native CPD engine (libcpd.so).
 *
 * The reference (eggeek/distributed-oracle-search) has no in-process FFI: its
 * hot path lives in the warthog executables `make_cpd_auto` and
 * `fifo_auto --alg table-search` (un-vendored submodule `pathfinding/`,
 * README.md:6-7, install.sh:3-7), driven over a process boundary by
 * make_cpds.py:20, make_fifos.py:21 and process_query.py:46,86-89.  This
 * header is the boundary our replacement executables (bin/make_cpd_auto,
 * bin/fifo_auto, bin/gen_distribute_conf) call, and the one a maintainer would
 * bind from Python (ctypes) or any other FFI.  Every
 * signature is plain C: pointers, sizes, status codes.  No torch types.
 *
 * Each entry point names the reference interface it replaces.  [U] marks
 * upstream-warthog behaviour that cannot be verified here (source absent,
 * SURVEY.md §0, §8c).
 *
 * Conventions
 *   - Node ids are the 0-based ids of the .xy file.  A "column" is a node's
 *     position in the DFS-preorder column order (warthog
 *     cpd::compute_dfs_preorder [U]); CPD runs store column indices.
 *   - Out-edge k of node n is the k-th `e n ...` line of the .xy file (file
 *     order); first moves are these k (0..14; 15 is reserved).
 *   - A run is `(start_column << 4) | move` (warthog rle_run32 [U]).
 *   - Every function returns CPD_OK (0) or a negative CPD_E_* code and sets a
 *     thread-local message readable with cpd_last_error().
 *   - Functions marked [host] never touch a GPU and work without one.
 *     Functions marked [gpu] fail loudly (CPD_E_HIP) when no gfx950 device is
 *     present; there is no CPU fallback in this library.
 */
#ifndef CPD_API_H
#define CPD_API_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CPD_OK          0
#define CPD_E_ARG      -1   /* bad argument / malformed input            */
#define CPD_E_HIP      -2   /* HIP runtime error or no usable device     */
#define CPD_E_OOM      -3   /* host or device allocation failed          */
#define CPD_E_NOROW    -4   /* a query's target has no row in the index  */
#define CPD_E_RANGE    -5   /* value out of supported range (degree>15,
                               distances >= 2^32-1, N >= 2^28)            */
#define CPD_E_IO       -6   /* file open/read/write/format error         */

#define CPD_PART_DIV    0
#define CPD_PART_MOD    1

#define CPD_MAX_DEGREE 15u          /* 4-bit move field, 0xF reserved [U] */
#define CPD_INF        0xFFFFFFFFu  /* unreachable distance              */
#define CPD_FM_ALL     0xFFFFu      /* wildcard first-move set           */

typedef struct cpd_plan  cpd_plan;   /* host-side preprocessing of one graph     */
typedef struct cpd_graph cpd_graph;  /* a plan resident on one GPU               */
typedef struct cpd_rows  cpd_rows;   /* a batch of built CPD rows (device)       */
typedef struct cpd_index cpd_index;  /* CPD rows loaded for table-search (device) */

/* Thread-local description of the last error. Never NULL. */
const char* cpd_last_error(void);
/* Library version string, e.g. "cpd-mi355x 0.1 gfx950". */
const char* cpd_version(void);

/* ------------------------------------------------------------------------ */
/* [host] Partitioner — replaces warthog util/distribution_controller.h,
 * exposed by ./bin/gen_distribute_conf (README.md:31-34,75-80;
 * process_query.py:46-53).  node -> (worker id, bucket id, index in bucket).
 *   mod: bid = node % key, bidx = node / key
 *   div: chunk = ceil(nodenum / key), bid = node / chunk, bidx = node % chunk
 *   both: wid = bid % maxworker                                   [U]        */
int cpd_partition(uint32_t nodenum, uint32_t maxworker, int method,
                  uint32_t key, uint32_t node,
                  uint32_t* wid, uint32_t* bid, uint32_t* bidx);
/* Number of buckets a (nodenum, method, key) partition has. */
int cpd_partition_nbuckets(uint32_t nodenum, int method, uint32_t key,
                           uint32_t* nbuckets);

/* [host] Disk preflight of a make_cpd_auto worker (make_cpds.py:58-60 starts
 * every worker at once, each writing its buckets into one --outdir; VERDICT
 * r05 item 2).  cpd_bucket_bytes: bytes of nrows compact rows at `bits` per
 * column (DOSCPD02/03) in nbuckets bucket files of `stripes` parts, headers
 * included.  cpd_space_check: CPD_E_IO (the numbers in cpd_last_error) when
 * the file system holding `dir` has fewer than `bytes` bytes available to
 * this user; *avail (may be NULL) = what it has.                             */
int cpd_bucket_bytes(uint32_t n, uint32_t bits, uint64_t nrows, uint32_t nbuckets,
                     uint32_t stripes, uint64_t* bytes);
int cpd_space_check(const char* dir, uint64_t bytes, uint64_t* avail);

/* [host] DFS-preorder column order — replaces warthog
 * cpd::compute_dfs_preorder [U]: iterative DFS from node 0 (then from every
 * still-unvisited node in id order), out-edges pushed in file order, so the
 * last out-edge is explored first.  order[node] = column.                    */
int cpd_dfs_preorder(uint32_t n, const uint32_t* row_ptr, const uint32_t* dst,
                     uint32_t* order);

/* [host] Synthetic grid-perturbed road graph.  W x H lattice,
 * jittered coordinates, random spanning tree kept bidirectional (strongly
 * connected), extra lattice edges (a share of them one-way) up to a mean
 * out-degree `mean_outdeg`; weights ceil(euclid * speed * asym / 10) in
 * [1, 65535]; node ids randomly permuted; out-edge order shuffled.
 * Call once with row_ptr == NULL to get *n and *m, then again with buffers
 * row_ptr[n+1], dst[m], w[m], x[n], y[n] (x / y may be NULL).               */
int cpd_synth_road_graph(uint32_t width, uint32_t height, double mean_outdeg,
                         uint64_t seed, uint32_t* n, uint32_t* m,
                         uint32_t* row_ptr, uint32_t* dst, uint32_t* w,
                         int32_t* x, int32_t* y);
/* The same generator with its departures from SURVEY.md §8(d) switchable:
 * flags = 0 is the §8(d) recipe as written (node id = row-major lattice cell,
 * every edge bidirectional, out-edges ordered east, north, west, south);
 * CPD_SYNTH_SHUFFLED (= what cpd_synth_road_graph builds) permutes node ids,
 * makes a fifth of the extra edges one-way and shuffles each out-edge list.
 * The shuffled edge order makes a reverse-CPD column's move (the column's own
 * out-edge index) uncorrelated with its neighbours', so rows compress
 * poorly; the direction order lets neighbouring columns share moves.        */
#define CPD_SYNTH_SHUFFLE_IDS   1u
#define CPD_SYNTH_SHUFFLE_EDGES 2u
#define CPD_SYNTH_ONE_WAY       4u
#define CPD_SYNTH_SHUFFLED      7u
int cpd_synth_road_graph_ex(uint32_t width, uint32_t height, double mean_outdeg,
                            uint64_t seed, uint32_t flags, uint32_t* n, uint32_t* m,
                            uint32_t* row_ptr, uint32_t* dst, uint32_t* w,
                            int32_t* x, int32_t* y);
/* [host] Congested weights (the `.diff` stand-in): a share
 * `frac` of the edges get w * U[lo, hi] rounded up; others unchanged.        */
int cpd_synth_congestion(uint32_t m, const uint32_t* w, double frac, double lo,
                         double hi, uint64_t seed, uint32_t* w_out);

/* ------------------------------------------------------------------------ */
/* [host] Preprocessing plan — the part of warthog's make_cpd_auto that runs
 * once per graph (graph load, column order) [U], plus what the GPU build needs
 * instead of a per-row Dijkstra: a contraction hierarchy (CH) with its
 * up/down sweep levels (GPHAST-style one-to-all sweeps).                     */
typedef struct cpd_plan_opts {
    int      threads;          /* OpenMP threads for the CH build (0 = all)  */
    uint32_t witness_settle;   /* witness-search settle limit (0 = default)  */
    int      verbose;          /* print CH progress to stderr                */
    int      no_hierarchy;     /* skip the CH: the plan can serve queries
                                  (fifo_auto) but cannot build rows         */
    int      ch_gpu;           /* 1: contract the CH on GPU ch_device (the
                                  host build's hierarchy, arc for arc;
                                  CPD_E_HIP without a GPU); 0: host threads */
    int      ch_device;
} cpd_plan_opts;

typedef struct cpd_plan_info {
    uint32_t n, m;
    uint64_t ch_up_arcs;       /* arcs v->x with rank(x) > rank(v)           */
    uint64_t ch_dn_arcs;       /* arcs u->v with rank(v) < rank(u)           */
    uint32_t levels_up;        /* launches of the upward sweep               */
    uint32_t levels_dn;        /* launches of the downward sweep             */
    uint64_t dist_bound;       /* proven upper bound on any finite distance  */
    double   ch_seconds;       /* wall time of the CH build                  */
} cpd_plan_info;

int  cpd_plan_create(const uint32_t* row_ptr, const uint32_t* dst,
                     const uint32_t* w, uint32_t n, uint32_t m,
                     const cpd_plan_opts* opts, cpd_plan** out);
/* The contraction alone, on a graph of any out-degree: a plan's limit of
 * CPD_MAX_DEGREE comes from the move field of its rows, and the contraction
 * meets far larger degrees in the overlay of any road graph.  The same two
 * builders under the same options (no_hierarchy is refused), but a GPU
 * contraction that fails is an error here, with no host build in its place.
 * The plan returned holds the hierarchy and nothing else: cpd_plan_info_get
 * (dist_bound 0), cpd_plan_export_ch and cpd_plan_free take it, every other
 * call refuses it with CPD_E_ARG.  For checks of the contraction.           */
int  cpd_hierarchy_create(const uint32_t* row_ptr, const uint32_t* dst,
                          const uint32_t* w, uint32_t n, uint32_t m,
                          const cpd_plan_opts* opts, cpd_plan** out);
int  cpd_plan_info_get(const cpd_plan* p, cpd_plan_info* info);
int  cpd_plan_order(const cpd_plan* p, uint32_t* order /* n */);
/* Export the hierarchy in NODE space (for CPU-side checks):
 * rank[n]; up CSR (up_off[n+1], up_dst, up_w); down CSR (dn_off[n+1],
 * dn_dst, dn_w); level_up[n], level_dn[n].  Any pointer may be NULL.        */
int  cpd_plan_export_ch(const cpd_plan* p, uint32_t* rank,
                        uint64_t* up_off, uint32_t* up_dst, uint32_t* up_w,
                        uint64_t* dn_off, uint32_t* dn_dst, uint32_t* dn_w,
                        uint32_t* level_up, uint32_t* level_dn);
/* save writes `path`.tmp.<pid>.<n> and renames it into place (atomic for
 * concurrent readers; concurrent savers of the same plan do not collide).
 * load checks the file's consistency: the column order is a permutation and
 * the hierarchy's arrays agree in size and range.                           */
int  cpd_plan_save(const cpd_plan* p, const char* path);
int  cpd_plan_load(const char* path, cpd_plan** out);
/* Load the plan cached at `path` if it was built from this very graph, else
 * build it and save it there.  make_cpds.py:58-60 starts every worker at once
 * (tmux -d) on one --outdir, so several processes may reach a cold cache
 * together: an exclusive flock(2) on `path`.lock lets one of them build while
 * the others wait and then load what it saved.  *status = 0 loaded, 1 built
 * and saved, 2 built but the cache could not be written (the plan is still
 * returned: a cache failure never fails the build).                         */
int  cpd_plan_cache(const char* path, const uint32_t* row_ptr, const uint32_t* dst,
                    const uint32_t* w, uint32_t n, uint32_t m, const cpd_plan_opts* opts,
                    cpd_plan** out, int* status);
void cpd_plan_free(cpd_plan* p);

/* ------------------------------------------------------------------------ */
/* [gpu] Devices and graphs. */
int  cpd_device_count(int* count);
/* Free and total HBM bytes of `device` (hipMemGetInfo there): what a caller
 * sizes cpd_graph_set_hbm_reserve against.                                 */
int  cpd_device_mem_info(int device, uint64_t* free_bytes, uint64_t* total_bytes);
/* HBM arena: commit `bytes` on `device` up front (touch != 0: also write
 * them once, paying first-touch costs now), for the library's device buffers
 * on that device to be carved from — so that a caller can overlap the
 * commit of a build's batch buffers (~200 GB: seconds) with other work, as
 * make_cpd_auto does with the plan.  Buffers carved from it are never
 * returned to it; cpd_device_arena_release frees the block, once the graphs,
 * rows and indexes using it are freed.  What does not fit is allocated
 * separately.  cpd_batch_bytes [host]: the HBM a build at `batch` rows needs
 * on a graph of n nodes and that max out-degree (an upper bound; graph
 * arrays excluded).                                                        */
int  cpd_device_arena(int device, uint64_t bytes, int touch);
int  cpd_device_arena_release(int device);
int  cpd_batch_bytes(uint32_t n, uint32_t max_degree, uint32_t batch, uint64_t* bytes);
/* Upload a plan to `device` (column-space CSR, CH arcs, levels). */
int  cpd_graph_create(const cpd_plan* p, int device, cpd_graph** out);
/* Batch width (rows built per sweep, multiple of 1024; 0 = auto from HBM). */
int  cpd_graph_set_batch(cpd_graph* g, uint32_t batch);
int  cpd_graph_get_batch(const cpd_graph* g, uint32_t* batch);
/* Bits per move of the graph's packed compact rows (cpd_rows_move_bits of
 * every cpd_rows it builds): 1, 2 or 4 for max out-degree <= 2, <= 4, else. */
int  cpd_graph_move_bits(const cpd_graph* g, uint32_t* bits);
/* HBM bytes the auto batch (batch 0) leaves free for what follows on this
 * GPU: an index built from the rows on the same handle, or a fifo_auto
 * serving beside a make_cpd_auto.  The auto batch takes 85% of the free HBM
 * above the reserve (default 0), both emit buffer sets included.  Takes
 * effect at the next cpd_graph_set_batch(g, 0), or at the first build when
 * the batch was never set.  With a reserve set, that call fails with
 * CPD_E_OOM when what is left cannot hold a 1024-row batch.  Explicit batch
 * widths ignore the reserve.                                               */
int  cpd_graph_set_hbm_reserve(cpd_graph* g, uint64_t bytes);
/* Optional node coordinates (x[n], y[n], node-id space, e.g. the .xy file's
 * `v id x y`; NULL clears them).  A batch's targets are then laid out over
 * the lanes along a Hilbert curve of their coordinates instead of by column,
 * so every 256-target lane group is spatially compact and its final
 * distances fit the narrow rows' 16-bit offsets.  Results are identical
 * either way; only the speed changes.                                      */
int  cpd_graph_set_coords(cpd_graph* g, const int32_t* x, const int32_t* y);
void cpd_graph_free(cpd_graph* g);

/* ------------------------------------------------------------------------ */
/* [gpu] CPD row build — replaces the per-source loop of warthog
 * make_cpd_auto (README.md:82-95; make_cpds.py:20): for each target t, the
 * distances d(n,t) for all n (reverse search: rows are keyed by target
 * because queries are routed to the worker owning t, process_query.py:56-57),
 * the first-move sets FM_t(n) = {k : w(n->v_k) + d(v_k,t) = d(n,t)}
 * (t itself and unreachable nodes: wildcard), and the greedy run-length row
 * over the DFS column order with the lowest-set-bit tie-break
 * (warthog graph_oracle::add_row [U]).  Rows stay in HBM in their compact
 * form — the RLE row expanded into a move per column (1, 2 or 4 bits by the
 * graph's max out-degree: cpd_graph_move_bits), which under the
 * greedy rule is a bijection (consecutive runs always carry different moves,
 * so the runs are column 0 and every column whose move differs from its left
 * neighbour's) — and are exported either as run words or in that form.
 * `reuse` (may be NULL) recycles a previous result's buffers.               */
int  cpd_build_rows(cpd_graph* g, const uint32_t* targets, uint32_t ntargets,
                    cpd_rows* reuse, cpd_rows** out);
/* The targets the NEXT cpd_build_rows call on g will start with (its first
 * batch; copied).  The current call's last batch then starts that batch's
 * up-sweep early, beside its own first moves and RLE count (a call with
 * several batches does this between its own batches without a hint).  A
 * next call with other targets discards the early work; results never
 * depend on the hint.  Cleared by every cpd_build_rows.                     */
int  cpd_graph_hint_next(cpd_graph* g, const uint32_t* targets, uint32_t ntargets);
int  cpd_rows_count(const cpd_rows* r, uint32_t* nrows, uint64_t* total_runs);
/* Run words (start_column << 4 | move), decoded on the GPU from the compact
 * rows: the rows of warthog's rle_run32 form [U], byte for byte.            */
int  cpd_rows_export(const cpd_rows* r, uint64_t* offsets /* nrows+1 */,
                     uint32_t* runs /* total_runs */);
/* Rows [first, first + count) of r: offsets relative to row `first`
 * (count + 1 values, offsets[0] = 0) and their runs.  Copies on a stream of
 * the calling thread's own, so exports from several host threads, and a
 * cpd_build_rows into ANOTHER cpd_rows on the same device, run concurrently
 * (the overlapped writer of bin/make_cpd_auto).  Either output may be NULL. */
int  cpd_rows_export_range(const cpd_rows* r, uint32_t first, uint32_t count,
                           uint64_t* offsets /* count+1 */, uint32_t* runs);
/* The compact form (DOSCPD02 bucket files, cpd_index_append_moves): a move
 * per column in *bits = 1, 2 or 4 bits — the fewest that hold every move of
 * the graph (a move indexes its column's out-list: out-degrees <= 2, <= 4,
 * else) — column c at bits bits*c .. bits*c + bits-1 of the row, a row being
 * *words = ceil(n * bits / 32) u32; the fields past column n-1 repeat the
 * last run's move.  Rows [first, first + count) back to back, on the calling
 * thread's stream (packed on the GPU when bits < 4).                        */
int  cpd_rows_move_words(const cpd_rows* r, uint32_t* words);
int  cpd_rows_move_bits(const cpd_rows* r, uint32_t* bits);
int  cpd_rows_export_moves(const cpd_rows* r, uint32_t first, uint32_t count,
                           uint32_t* moves /* count * words */);
int  cpd_rows_targets(const cpd_rows* r, uint32_t* targets /* nrows */);
/* The batch lane each row was built in (lane = position in its sweep batch,
 * 0..batch-1; rows are lane-sorted by Hilbert key with coordinates, else by
 * column).  Results never depend on it; tests use it to cover every slab.   */
int  cpd_rows_lanes(const cpd_rows* r, uint32_t* lanes /* nrows */);
/* [gpu] Page-locked host memory for export destinations: a D2H copy into it
 * runs at PCIe rate (a pageable destination is staged through a bounce
 * buffer at a fraction of it).  Free with cpd_host_free.                    */
int  cpd_host_alloc(size_t bytes, void** out);
void cpd_host_free(void* p);
/* Wait for the device work behind r: a build returns once its rows' run
 * counts are known, while the last batch's run emit may still be running
 * (it overlaps the next build's sweeps); every accessor above waits for it,
 * this call only waits.  The bench calls it inside its timed region. */
int  cpd_rows_wait(const cpd_rows* r);
void cpd_rows_free(cpd_rows* r);

/* [gpu] Inspection (tests): distances d(n,t) in NODE order, n-major
 * (dist[node * ntargets + i]), and first-move sets fm[i * n + node].
 * ntargets <= batch.  Either output may be NULL.                            */
int  cpd_debug_rows(cpd_graph* g, const uint32_t* targets, uint32_t ntargets,
                    uint32_t* dist, uint16_t* fm);

/* ------------------------------------------------------------------------ */
/* [gpu] Table-search index — replaces fifo_auto's CPD load + `--alg
 * table-search` extraction (make_fifos.py:20-21; README.md:110).            */
int  cpd_index_create(cpd_graph* g, const uint32_t* row_targets, uint32_t nrows,
                      const uint64_t* offsets, const uint32_t* runs,
                      cpd_index** out);
/* Same, straight from device-resident rows (no host round trip). */
int  cpd_index_from_rows(cpd_graph* g, const cpd_rows* r, cpd_index** out);

/* Streamed index — the load of fifo_auto (make_fifos.py:21 loads every CPD
 * the worker owns; README.md:110).  Declare the rows (row i = target
 * row_targets[i]) and their total run count, then append the rows in order,
 * in chunks, from host arrays (a bucket file read piece by piece) or from a
 * device-built cpd_rows; queries need every row appended.  The mode is fixed
 * at creation: DENSE (or AUTO resolving to it: 4 * total_runs > n/2 * nrows)
 * expands each chunk into the 4-bit move tables as it arrives and keeps no
 * runs, so HBM holds nrows * n/2 bytes however large the runs are; RLE keeps
 * the runs (total_runs of capacity).  Dense tables hold a move per column
 * at the graph's packed width (cpd_graph_move_bits: 1, 2 or 4 bits; nrows *
 * npad * bits / 8 bytes).  Appended host rows are format-checked on the GPU
 * (first run at column 0, columns increasing and < n; for tables narrower
 * than 4 bits also every move < 2^bits), CPD_E_ARG otherwise.                */
int  cpd_index_create_empty(cpd_graph* g, const uint32_t* row_targets, uint32_t nrows,
                            int mode, uint64_t total_runs, cpd_index** out);
/* offsets: count + 1 values relative to the chunk (offsets[0] = 0). */
int  cpd_index_append_rows(cpd_index* ix, uint32_t count, const uint64_t* offsets,
                           const uint32_t* runs);
int  cpd_index_append_built_rows(cpd_index* ix, const cpd_rows* r);
/* Rows in the compact form (cpd_rows_export_moves layout: count rows of
 * ceil(n * bits / 32) words, bits = 1, 2 or 4): copied into a DENSE index's
 * tables when bits is the graph's packed width, else repacked on the GPU
 * (wider rows must carry moves that fit: CPD_E_ARG otherwise), or decoded
 * into run words for an RLE index (total_runs of the create call must cover
 * them).  No other check is needed: a move naming no out-edge of its column
 * stops a walk there, unfinished, as the oracle's walk does.               */
int  cpd_index_append_moves(cpd_index* ix, uint32_t count, uint32_t bits, const uint32_t* moves);
/* Rows declared / appended, runs resident in HBM, bytes of dense tables.     */
int  cpd_index_info(const cpd_index* ix, uint32_t* nrows, uint32_t* added,
                    uint64_t* runs_resident, uint64_t* dense_bytes);

/* In-HBM representation the extraction walks.  RLE: binary search in the run
 * rows (galloping from the previous move's run).  DENSE: the rows expanded on
 * the GPU into 4-bit move tables (n/2 bytes per row, one load per move) —
 * the same move for every column, so identical results.  AUTO (default)
 * picks the smaller of the two (reverse-CPD rows on road graphs often hold
 * more than n/8 runs, where the dense table is smaller AND faster).
 * get_mode reports the representation AUTO resolves to.                     */
#define CPD_INDEX_AUTO  0
#define CPD_INDEX_RLE   1
#define CPD_INDEX_DENSE 2
int  cpd_index_set_mode(cpd_index* ix, int mode);
int  cpd_index_get_mode(const cpd_index* ix, int* mode);
/* Edge weights used for path cost (m entries, original edge order):
 * NULL restores the free-flow weights; otherwise e.g. the .diff weights
 * (process_query.py:89,178 sends the diff name with every batch).           */
int  cpd_index_set_weights(cpd_index* ix, const uint32_t* w);

typedef struct cpd_query_stats {
    uint64_t queries;
    uint64_t finished;      /* queries whose walk reached t                  */
    uint64_t hops;          /* sum of moves taken (n_expanded / plen)        */
    uint64_t cost;          /* sum of path costs                             */
    double   kernel_ms;     /* device time of the extraction kernel          */
} cpd_query_stats;

/* Walk each query s -> t by repeated get_move(t, cur) (binary search in
 * row(t) at column(cur), warthog graph_oracle::get_move [U]) and sum the
 * selected weights.  k_moves < 0: walk to t (process_query.py:153 sends -1);
 * otherwise stop after k moves.  cost/hops/finished may be NULL.
 * Returns CPD_E_NOROW if some t has no row in this index.                    */
int  cpd_query_batch(cpd_index* ix, const uint32_t* s, const uint32_t* t,
                     uint32_t nq, int32_t k_moves, uint64_t* cost,
                     uint32_t* hops, uint8_t* finished, cpd_query_stats* st);
/* The same in three steps, so that a caller can keep the queries resident in
 * HBM and time the extraction alone: prepare uploads (s, t) as columns,
 * run launches the kernel (stats only), fetch copies per-query results.     */
int  cpd_query_prepare(cpd_index* ix, const uint32_t* s, const uint32_t* t,
                       uint32_t nq);
int  cpd_query_run(cpd_index* ix, int32_t k_moves, cpd_query_stats* st);
int  cpd_query_fetch(cpd_index* ix, uint64_t* cost, uint32_t* hops,
                     uint8_t* finished);
/* The walks of the last cpd_query_prepare, with their nodes: the sequence the
 * repeated graph_oracle::get_move [U] walk visits, which the reference's
 * workers only sum up — and, with k_moves = k (process_query.py:153 k_moves,
 * args.py -k: "extract the first k moves, then replan"), the node where the
 * walk stopped.  Path q is s[q], then the node reached by each move:
 * hops[q] + 1 node ids (.xy ids, not columns), ending at t[q] when
 * finished[q], else at the node where the walk stopped (k_moves reached, a
 * move naming no out-edge, or the n-move loop guard).  offsets: nq + 1 values
 * in the CALLER's query order, offsets[0] = 0, offsets[q+1] - offsets[q] =
 * hops[q] + 1; the nodes stay in HBM (4 * offsets[nq] bytes; CPD_E_OOM naming
 * them when they do not fit — the index and the prepared queries stay usable)
 * until the next prepare / run / paths call on ix.  Also does what
 * cpd_query_run does (st, and cpd_query_fetch afterwards returns this walk's
 * cost / hops / finished).  The nodes never depend on the weights
 * (cpd_index_set_weights), only cost does.  This is always the table-search
 * walk: the paths of a preceding cpd_query_search are NOT what it returns
 * (cpd_query_search_paths returns those).
 * Known limit, inherited from the walk kernel (cpd_query_run has it too): in
 * a batch large enough for a wave's lanes to be refilled (more than 65536
 * queries on a dense index, 524288 on an RLE one) a refilled lane takes one
 * move before k_moves is checked, so with k_moves = 0 such a query reports
 * hops = 1 and a 2-node path instead of 0 and [s]; k_moves >= 1 and < 0 are
 * exact at every size, and hops, cost and the path always agree.
 * When a device arena is committed the node buffer is carved from it; the
 * arena never takes a buffer back, so each batch with more nodes than any
 * before it on this index uses up that many more arena bytes until
 * cpd_device_arena_release (what does not fit is allocated separately).     */
int  cpd_query_paths(cpd_index* ix, int32_t k_moves, uint64_t* offsets /* nq+1 */,
                     cpd_query_stats* st);
/* Path nodes of queries [first, first + count) of the caller's order, back to
 * back: offsets[first+count] - offsets[first] values — the paths of the last
 * cpd_query_paths or cpd_query_search_paths on the prepared queries.
 * CPD_E_ARG before any of the two on the prepared queries, or for a range
 * past nq.                                                                   */
int  cpd_query_paths_fetch(cpd_index* ix, uint32_t first, uint32_t count, uint32_t* nodes);

/* Costs under several weight sets in ONE walk — what the reference pays one
 * experiment per diff for (process_query.py:178 sends the whole scenario to
 * the workers again for every congestion file of `diffs`; args.py -k: "extract
 * the first k moves, then replan" under the next one).  The table-search
 * route never depends on the weights, so the walk is taken once and every
 * edge on it is summed under each set.
 * cpd_index_set_weight_sets: nsets (<= CPD_MAX_WEIGHT_SETS) arrays of m
 * weights in original edge order, as cpd_index_set_weights takes one; w[j] ==
 * NULL = the free-flow weights (the "-" diff); nsets == 0 clears the sets.
 * CPD_E_ARG for more sets, or w == NULL with nsets > 0.  The sets are copied,
 * permuted to column space and kept in HBM — 16 B per adjacency slot for up
 * to 4 sets, 32 B above — until replaced, cleared or cpd_index_free.  They
 * are independent of the index's current weights: cpd_index_set_weights,
 * cpd_query_run, cpd_query_paths and cpd_query_search neither see nor change
 * them, and a call here leaves the search's tables as they are.
 * cpd_query_costs: on the queries of the last cpd_query_prepare, the walk of
 * cpd_query_run (k_moves with its meaning, the n-move loop guard, and the
 * k_moves = 0 refill limit described at cpd_query_paths).
 *   slice_moves == 0: the cost of every walk under every set, C = nsets
 *     values per query;
 *   slice_moves == S > 0: C = 1 value per query; move number h of the walk
 *     (0-based) is costed under set min(h / S, nsets - 1): the cost of a trip
 *     replanned every S moves under successive weight sets.
 * st: queries / finished / hops as cpd_query_run reports them, cost = the sum
 * of set 0's column (slice_moves == 0) or of the one column, kernel_ms of
 * this walk.  CPD_E_ARG when no sets are loaded or the index is incomplete.
 * The results live in buffers of their own: what cpd_query_fetch and
 * cpd_query_paths_fetch return is left as it was.
 * cpd_query_costs_fetch: costs[q * C + j] in the CALLER's query order (sums
 * are 64-bit: weights up to 0xFFFFFFFF never wrap), hops and finished as the
 * walk's; any pointer may be NULL; scattered to the caller's order on the GPU
 * as cpd_query_fetch does.  CPD_E_ARG before a cpd_query_costs on the
 * prepared queries.
 * When a device arena is committed the set table and the result buffers are
 * carved from it; the arena never takes a buffer back, so a table or batch
 * larger than any before it on this index uses up that many more arena bytes
 * until cpd_device_arena_release (what does not fit is allocated separately). */
#define CPD_MAX_WEIGHT_SETS 8u
int  cpd_index_set_weight_sets(cpd_index* ix, uint32_t nsets, const uint32_t* const* w);
int  cpd_query_costs(cpd_index* ix, int32_t k_moves, uint32_t slice_moves, cpd_query_stats* st);
int  cpd_query_costs_fetch(cpd_index* ix, uint64_t* costs, uint32_t* hops, uint8_t* finished);

/* Edge loads — how much demand every edge carries when a batch of queries is
 * routed: the quantity a congestion diff is made from (the reference takes
 * its `diffs` as given, process_query.py:178; nothing in it produces them).
 * cpd_query_loads: on the queries of the last cpd_query_prepare, the walk of
 * cpd_query_run (k_moves with its meaning, the n-move loop guard, and the
 * k_moves = 0 refill limit described at cpd_query_paths).  For every move a
 * walk takes, demand[q] (nq values in the CALLER's query order; NULL = 1 for
 * every query) is added to the counter of (slice j, edge e):
 *   e  the original index of the out-edge taken — its position in the .xy
 *      file order, the index cpd_index_set_weights uses (parallel edges are
 *      told apart);
 *   j  min(h / slice_moves, nslices - 1) for move number h of the walk
 *      (0-based); j = 0 when nslices == 1.  The load per congestion state of
 *      a trip replanned every slice_moves moves, the counterpart of
 *      cpd_query_costs' sliced mode.
 * A move that names no out-edge ends the walk and adds nothing; a walk that
 * stops unfinished (k_moves, the loop guard) has loaded the moves it took.
 * Counters are 64-bit: a demand of 0xFFFFFFFF on every query never wraps.
 * Integer adds commute, so the table is exact and the same in every run; it
 * never depends on the weights.
 * flags = 0: the table is zeroed first.  CPD_LOADS_ACCUMULATE: the call adds
 * to what earlier calls on this index left (nothing: it starts from zero),
 * across cpd_query_prepare calls — a demand set larger than a batch goes
 * through in pieces, and workers' tables add up on the head; CPD_E_ARG when
 * nslices or slice_moves differ from the resident table's, or that table is
 * a timed walk's (cpd_query_timed).
 * Also does what cpd_query_run does (st, and cpd_query_fetch afterwards
 * returns this walk's cost / hops / finished under the index's current
 * weights) and, like it, ends the validity of fetched paths.
 * CPD_E_ARG when nslices is 0 or above CPD_MAX_LOAD_SLICES, slice_moves is 0
 * with nslices > 1 or non-zero with nslices == 1, or the index is incomplete.
 * cpd_query_loads_fetch: loads[j * m + e], nslices * m values, permuted from
 * the table's adjacency-slot order to original edge order on the GPU and
 * copied out once.  CPD_E_ARG before any cpd_query_loads on the index, or
 * after a clear.
 * The table (8 B per slice and adjacency slot: n x 1, 2, 4, 8 or 16 slots
 * by the graph's largest out-degree) lives in HBM until cpd_query_loads_clear
 * or cpd_index_free.  cpd_index_set_weights, the weight sets,
 * cpd_query_paths, cpd_query_costs and cpd_query_search neither see nor
 * change it.  When a device arena is committed the table is carved from it;
 * the arena never takes a buffer back, so a table larger than any before it
 * on this index (or one made again after a clear) uses up that many more
 * arena bytes until cpd_device_arena_release (what does not fit is allocated
 * separately).                                                              */
#define CPD_MAX_LOAD_SLICES 8u
#define CPD_LOADS_ACCUMULATE 1u
int  cpd_query_loads(cpd_index* ix, int32_t k_moves, const uint32_t* demand /* nq, caller order; NULL = 1 each */,
                     uint32_t nslices /* 1..8 */, uint32_t slice_moves /* 0 iff nslices == 1 */,
                     uint32_t flags, cpd_query_stats* st);
int  cpd_query_loads_fetch(cpd_index* ix, uint64_t* loads /* nslices * m */);
int  cpd_query_loads_clear(cpd_index* ix);

/* Timed walks — the time axis of the two above.  cpd_query_costs' sliced mode
 * and cpd_query_loads pick the congestion state of a move by its move NUMBER;
 * a weight set is the state of the network during an interval of TIME (the
 * reference is a "Time-Dependant-Oracle-Search", process_query.py:250).  Here
 * every query carries a clock that starts at its departure and advances with
 * the cost being summed, and a move is costed — and loaded — under the set of
 * the interval in which its edge is entered.
 * cpd_query_timed: on the queries of the last cpd_query_prepare, the walk of
 * cpd_query_run (k_moves with its meaning, the n-move loop guard, the rule
 * that a move naming no out-edge stops the walk, and the k_moves = 0 refill
 * limit described at cpd_query_paths); the route never depends on the
 * weights.  With the K sets W_0 .. W_{K-1} of cpd_index_set_weight_sets, a
 * period P (in weight units) and tau_0 = depart[q] (nq values, u64, weight
 * units, the CALLER's query order; NULL = 0 for every query), move number h
 * on original edge e_h does
 *     j_h       = min(tau_h / P, K - 1)   (integer division: tau_h == k P
 *                                          belongs to set k)
 *     c_h       = W_{j_h}[e_h]
 *     tau_{h+1} = tau_h + c_h
 * — the weight is frozen when the edge is entered (piecewise constant; one
 * heavy edge may cross several periods).  Per query cost = tau_end - depart[q]
 * (u64), hops and finished as the plain walk's.  K = 1, or P beyond every
 * arrival, is cpd_query_costs' column 0.
 * flags & CPD_TIMED_LOADS: demand[q] (nq values, caller order; NULL = 1 each;
 * not read without the flag) is added to counter (j_h, e_h) of the index's
 * load table for every move taken: K planes of m 64-bit counters, e the
 * original edge index as in cpd_query_loads, fetched by cpd_query_loads_fetch
 * (K * m values) and dropped by cpd_query_loads_clear.  The table remembers
 * its kind: without CPD_LOADS_ACCUMULATE it is made again and zeroed; with it
 * the resident table must be a timed one of the same K and period (none
 * resident: the call starts from zero), else CPD_E_ARG and the table stays —
 * and cpd_query_loads(.., CPD_LOADS_ACCUMULATE) onto a timed table is
 * CPD_E_ARG too.  Load the demand per interval here, turn the loads into
 * weight sets, cost the demand again: a traffic-assignment loop.
 * P must be in [1, 2^60] and every departure below 2^63 (a walk adds less
 * than n < 2^28 moves x 2^32, so the clock and (j + 1) P never wrap):
 * CPD_E_ARG otherwise, the message naming the first offending value.
 * CPD_E_ARG also when no sets are loaded, the index is incomplete, or
 * CPD_LOADS_ACCUMULATE comes without CPD_TIMED_LOADS.
 * st: queries / finished / hops as cpd_query_run reports them, cost = the sum
 * of the costs, kernel_ms of this walk.  The results live in buffers of their
 * own: what cpd_query_fetch, cpd_query_paths_fetch and cpd_query_costs_fetch
 * return is left as it was, and fetched paths stay valid.
 * cpd_query_timed_fetch: cost / hops / finished in the CALLER's query order;
 * any pointer may be NULL; scattered to the caller's order on the GPU as
 * cpd_query_costs_fetch does.  CPD_E_ARG before a cpd_query_timed on the
 * prepared queries.  Both answer the empty batch.
 * Arena: the result buffers and the table are carved as cpd_query_costs' and
 * cpd_query_loads' are.                                                     */
#define CPD_TIMED_LOADS 2u        /* a bit of its own beside CPD_LOADS_ACCUMULATE */
int  cpd_query_timed(cpd_index* ix, int32_t k_moves,
                     const uint64_t* depart /* nq, caller order; NULL = 0 */, uint64_t period,
                     const uint32_t* demand /* nq; NULL = 1; read only with CPD_TIMED_LOADS */,
                     uint32_t flags /* CPD_TIMED_LOADS | CPD_LOADS_ACCUMULATE */,
                     cpd_query_stats* st);
int  cpd_query_timed_fetch(cpd_index* ix, uint64_t* cost, uint32_t* hops, uint8_t* finished);
void cpd_index_free(cpd_index* ix);

/* [gpu] CPD-heuristic search — fifo_auto's other algorithm family
 * (args.py:29-57 --h-scale / --f-scale / -k / time
 * limits, worker JSON keys hscale, fscale, time, itrs, k_moves,
 * process_query.py:149-160).  warthog's cpd_search is absent: the semantics
 * are restated in oracle/cpd_oracle.c (ora_cpd_search) [U].  A* from s under
 * the index's current weights (cpd_index_set_weights), heuristic hscale x the
 * free-flow cost of the CPD path to t, incumbent from the CPD path's cost
 * under the current weights (only paths of <= k_moves moves when k_moves >=
 * 0); stops when f_min x (1 + fscale) >= incumbent, after itrs expansions,
 * or once time_ns have elapsed.  Runs on the queries of the last
 * cpd_query_prepare; per query results (cost, plen as hops, finished) via
 * cpd_query_fetch.  The CPD path values (heuristic, incumbent) come from
 * per-row tables — 20 B per column per index row, built once per index and
 * per weights by pointer jumping — when those fit in half of the free HBM
 * (tables = CPD_SEARCH_AUTO) or when asked for (_TABLES, CPD_E_OOM if they do
 * not fit); else (_WALKS, or AUTO on a large index) from CPD walks memoised
 * in each search's workspace, so an index of any size can be searched.  The
 * results and counters are the same either way.  A search's workspace holds
 * `capacity` columns (searched ones; with walks also the walked ones; 72 /
 * 120 B each).  Before each pop a search checks that the expansion fits;
 * when it might not, it stops there with its state whole and (when a
 * larger pass can follow) copies it into a spill pool; the next pass, at
 * 4x the capacity, resumes it from there — same pops, counters and results
 * as one uninterrupted search (a search whose record finds the pool full
 * restarts from scratch instead; `wasted_expanded` counts that work).  What
 * still overflows at capacity_max (or when no larger workspace fits in
 * HBM) stops unfinished, with finished = 2 in cpd_query_fetch, and is
 * counted in `overflow`.  capacity = 0 selects the library's workspace
 * policy (what fifo_auto runs): the first pass at 2^13 columns when fscale
 * > 0 with tables (2^14 with walks) and 2^14 at fscale 0, lowered (to 2^10
 * at most) until every query of
 * the request gets a lane; capacity_max 0 = 4 n rounded up to a power of 2
 * (<= 2^24); workspace_frac 0 = 0.85 of the free HBM.  An explicit capacity
 * keeps capacity_max 0 = no larger pass and workspace_frac 0 = 0.25.  The
 * time limit is wall clock (as fifo_auto runs it);
 * virtual_tick_ns > 0 replaces it by a deterministic clock that advances
 * virtual_tick_ns per expansion and per edge touched (the oracle's
 * restatement, for tests).                                                   */
#define CPD_SEARCH_AUTO   0
#define CPD_SEARCH_TABLES 1
#define CPD_SEARCH_WALKS  2
typedef struct cpd_search_opts {
    double   hscale;       /* 1.0 */
    double   fscale;       /* 0.0 */
    int32_t  k_moves;      /* -1: whole CPD paths */
    int64_t  itrs;         /* -1: no expansion limit */
    uint64_t time_ns;      /* 0: no time limit (per query) */
    uint32_t capacity;     /* columns per search, power of 2 (0 = automatic) */
    uint64_t virtual_tick_ns; /* 0: wall-clock time limit; else virtual clock */
    int32_t  tables;       /* CPD_SEARCH_AUTO / _TABLES / _WALKS             */
    double   workspace_frac; /* share of the free HBM the lanes' workspaces and
                                spill pools may take (0 = automatic / 0.25);
                                more lanes search at once                    */
    uint32_t capacity_max; /* 0: automatic / none; else searches that overflow
                              `capacity` continue in later passes at 4x the
                              capacity (fewer lanes) up to capacity_max: many
                              lanes for the common short searches, the big
                              workspace only for the long ones              */
} cpd_search_opts;

typedef struct cpd_search_stats {
    uint64_t queries, finished, expanded, inserted, touched, updated, surplus, plen, overflow;
    double   kernel_ms;    /* device time of the search kernel              */
    uint64_t lanes;        /* concurrent searches (workspace slots)         */
    double   tables_ms;    /* device time spent (re)building the tables     */
    int32_t  tables;       /* the form used: CPD_SEARCH_TABLES or _WALKS    */
    uint64_t reruns;       /* searches run again at a larger capacity       */
    uint64_t resumed;      /* ... of them continued from a spilled state    */
    uint64_t restarted;    /* ... of them started over (spill pool full)    */
    uint64_t wasted_expanded; /* expansions the restarted ones threw away  */
    uint32_t passes;       /* search kernel launches (1 + escalations)      */
    uint32_t capacity;     /* columns per lane of the first pass            */
    uint32_t capacity_last;/* ... of the last pass                          */
} cpd_search_stats;

int  cpd_query_search(cpd_index* ix, const cpd_search_opts* opts, cpd_search_stats* st);
/* Per-query counters of the last search: counters[5 q + k] = expanded,
 * inserted, touched, updated, surplus of query q (caller order).            */
int  cpd_query_search_counters(cpd_index* ix, uint32_t* counters);

/* cpd_query_search with the nodes of every route found.  The incumbent of a
 * search is "the A* tree from s to the node v* whose expansion last lowered
 * it, then the row's CPD walk from v* to t"; path q is that route, read when
 * the search has ended (in whatever pass it ends):
 *   prefix  the parent chain v* -> par(v*) -> ... -> s, reversed; par(u) is
 *           the node whose relaxation last set g(u) (the insert or a strictly
 *           smaller update), so the chain is a tree path;
 *   suffix  the table-search walk from v* to t, lw(v*) moves, without v*.
 * finished = 1: prefix nodes + lw(v*) node ids (.xy ids) from s to t, [s]
 * when s == t; finished = 0 (no incumbent) or 2 (stopped on the workspace):
 * 0 nodes.  offsets: nq + 1 values in the CALLER's order, offsets[0] = 0;
 * the nodes stay in HBM for cpd_query_paths_fetch, in the index's path
 * buffer (as cpd_query_paths: from the arena when one is committed;
 * CPD_E_OOM naming the bytes when they do not fit), until the next prepare /
 * run / paths / search_paths call on ix.
 * The path's cost under the index's current weights is <= the reported cost:
 * equal, with hops[q] moves, whenever the heuristic is consistent (hscale <=
 * 1 and every selected weight >= its free-flow weight: nodes are never
 * re-opened); with hscale > 1 a chain node's g may have improved after the
 * incumbent was set, and the path returned is that cheaper chain, whose move
 * count may differ from hops[q] (a search that runs until its stop rule ends
 * it has expanded every re-opened chain node again: this needs itrs or the
 * time limit to end it in between).  cost / hops / finished of cpd_query_fetch,
 * the counters and st stay the oracle's (cpd_query_search's) in every case.
 * Each search writes its prefix into a pool of prefix_bytes bytes in HBM
 * (4 per node; info->prefix_nodes nodes over all queries).  0 = automatic:
 * the smaller of 4 * nq * n bytes (no prefix is longer than n nodes) and
 * 1/32 of the free HBM, taken before the workspace is sized; the share is
 * a policy, not a measured optimum.  When the pool is too small the call
 * returns CPD_E_OOM and the message names the bytes needed (info
 * ->prefix_nodes * 4): the search's cost / hops / finished / counters are
 * whole and fetchable, the index and the prepared queries stay usable, and a
 * second call with at least that many bytes succeeds.  The workspace costs 8
 * B more per column of capacity (80 / 128 B) than cpd_query_search's.
 * Does everything cpd_query_search does (st; cpd_query_fetch and
 * cpd_query_search_counters afterwards).                                     */
typedef struct cpd_search_paths_info {
    uint64_t nodes;          /* offsets[nq]                                   */
    uint64_t prefix_nodes;   /* summed over the queries: what the pool had to hold */
    uint64_t prefix_bytes;   /* the pool's size used for this call            */
    double   paths_ms;       /* device time of suffix walk + offsets + join   */
} cpd_search_paths_info;
int  cpd_query_search_paths(cpd_index* ix, const cpd_search_opts* opts,
                            uint64_t prefix_bytes /* 0 = automatic */,
                            uint64_t* offsets /* nq + 1, caller order */,
                            cpd_search_stats* st, cpd_search_paths_info* info);

/* cpd_query_search with the edge loads of every route found — what closes the
 * traffic-assignment loop of cpd_query_loads / cpd_query_timed: their walk
 * never depends on the weights, so a second iteration would load the edges
 * the first did; the route a search finds under cpd_index_set_weights does
 * react to congestion.  On the queries of the last cpd_query_prepare, for
 * every query that ends with finished = 1, demand[q] (nq values, the CALLER's
 * order; NULL = 1 each) is added to the 64-bit counter of each edge of its
 * route — the route cpd_query_search_paths returns, read when the search has
 * ended (with its hscale > 1 caveat); finished = 0 or 2 adds nothing.  The
 * edge of each move, parallel edges told apart (original edge index, as
 * cpd_query_loads counts):
 *   prefix move p -> u (u's parent is p in the chain s ... v*): among the
 *           out-edges of p with head u, the one of least weight under the
 *           index's current weights, on ties the first in p's out-list (file
 *           order).  This is the edge whose relaxation set g(u): a relaxation
 *           scans the out-list in order and replaces g only by a strictly
 *           smaller value;
 *   suffix move (the CPD walk from v* to t, lw(v*) moves): the edge the row's
 *           move names, what cpd_query_loads counts — the edge the reported
 *           cost was summed over, though a parallel one may be cheaper under
 *           the current weights.
 * The table is the index's resident load table, one plane, the kind
 * cpd_query_loads(nslices = 1) fills: cpd_query_loads_fetch returns its m
 * values, cpd_query_loads_clear drops it.  flags = 0 makes and zeroes it;
 * CPD_LOADS_ACCUMULATE adds to a resident one-plane table (none resident: it
 * starts from zero) — one that cpd_query_loads(nslices = 1) filled too: an
 * all-or-nothing start, then search iterations; CPD_E_ARG when the resident
 * table is sliced or a timed walk's, the table stays.  CPD_E_ARG also for
 * unknown flag bits and for an incomplete index.
 * Does everything cpd_query_search does (st; cpd_query_fetch and
 * cpd_query_search_counters afterwards, the oracle's) and, like cpd_query_run,
 * ends the validity of fetched paths; it builds no node buffer.  The prefix
 * pool is cpd_query_search_paths' (prefix_bytes, 0 = automatic): when it is
 * too small the call returns CPD_E_OOM naming the bytes needed, the search's
 * results are whole and fetchable, the load table is as it was before the
 * call, and a second call with that many bytes succeeds.  The empty batch is
 * answered: the table zeroed or kept, info all 0.
 * The table is carved from the arena as cpd_query_loads' is.                 */
typedef struct cpd_search_loads_info {
    uint64_t moves;          /* counter adds made: prefix moves + suffix moves over all routes */
    uint64_t prefix_moves;   /* ... of them on A*-tree edges                  */
    uint64_t prefix_nodes;   /* as cpd_search_paths_info                      */
    uint64_t prefix_bytes;   /* as cpd_search_paths_info                      */
    double   loads_ms;       /* device time of the two load launches          */
} cpd_search_loads_info;
int  cpd_query_search_loads(cpd_index* ix, const cpd_search_opts* opts,
                            uint64_t prefix_bytes /* 0 = automatic */,
                            const uint32_t* demand /* nq, caller order; NULL = 1 each */,
                            uint32_t flags /* 0 | CPD_LOADS_ACCUMULATE */,
                            cpd_search_stats* st, cpd_search_loads_info* info);

/* ------------------------------------------------------------------------ */
/* [gpu] The assignment loop — loads to weights in HBM, iterated with
 * cpd-search.  cpd_query_loads / cpd_query_timed / cpd_query_search_loads
 * leave edge loads in the index's resident table; the step below turns them
 * into weights without leaving HBM (the load table, the free-flow adjacency,
 * the selected adjacency and the weight-set table all index an adjacency slot
 * the same way, so the update is slot-wise: no permutation, no host copy),
 * and cpd_query_assign iterates search, load and update.  The reference takes
 * its congestion `diffs` as given (process_query.py:178); nothing in it makes
 * them.
 *
 * The delay function.  Integer arithmetic, every intermediate fits 64 bits.
 * For an edge with free-flow weight w0, capacity c >= 1 and load counter L:
 *     x   = L / load_div
 *     r   = (x >= ((u64)c << 4)) ? (1 << 20) : ((x << 16) / c)
 *                                   the ratio x / c in Q16, clamped at 16.0
 *     p   = r;  repeat power - 1 times:  p = (p * r) >> 16        p <= 2^32
 *     t   = (w0 * p) >> 16
 *     add = (t * a_num) / a_den
 *     w'  = min(w0 + add, 0xFFFFFFFF)   in mathematical integers: the sum is
 *                                        never allowed to wrap
 * All divisions truncate.  w0 is always the FREE-FLOW weight, never the
 * current one: the update does not compound.  L = 0 gives w' = w0, and w' >=
 * w0 always, so the search's heuristic stays consistent for hscale <= 1.
 * Adjacency slots past a column's out-degree are copied unchanged: a move
 * that names no out-edge still stops a walk.  BPR is a = 3/20, power 4;
 * load_div is the number of all-or-nothing loadings the counters sum (x =
 * their mean). */
typedef struct cpd_vdf {
    uint32_t a_num;    /* 0..65535 */
    uint32_t a_den;    /* 1..65535 */
    uint32_t power;    /* 1..4 */
    uint32_t load_div; /* >= 1 */
} cpd_vdf;

typedef struct cpd_vdf_info {
    uint64_t tstt_lo, tstt_hi; /* sum over edges and planes of x * w', 128 bits (mod 2^128) */
    uint64_t changed;          /* (plane, edge) pairs with w' != w0 */
    uint32_t planes;           /* planes of the table read */
    double   vdf_ms;           /* device time of the capacity permutation + the update */
} cpd_vdf_info;

/* Weights from the resident load table.  capacity: m values in original edge
 * order, each >= 1.  What is written depends on the table's kind:
 *   one plane (cpd_query_loads with nslices = 1, cpd_query_search_loads): the
 *       index's CURRENT weights, w' on every edge — the state
 *       cpd_index_set_weights(w') leaves (the search's incumbent tables are
 *       rebuilt at the next search); cpd_index_set_weights(ix, NULL) still
 *       restores free flow;
 *   K >= 2 planes (sliced cpd_query_loads, cpd_query_timed with
 *       CPD_TIMED_LOADS): weight set j from plane j, K sets, as
 *       cpd_index_set_weight_sets(K, ..) would hold them; the current weights
 *       and the search's tables are left as they were.
 * The load table is only read.  The update and the 128-bit sum are one kernel
 * pass over the slots; integer adds commute, so info is exact and the same in
 * every run.  The capacities are uploaded and permuted to slot order by a
 * small kernel on every call (4 m bytes; no copy is kept between calls, so a
 * caller may change them freely).
 * CPD_E_ARG, naming the first offending value: no resident table, an
 * incomplete index, capacity NULL or some capacity 0, a_num > 65535, a_den or
 * power out of range, load_div 0.  On error the table, the weights and the
 * sets are untouched.  info may be NULL.  The buffers are carved from the
 * arena as the load table is.                                                */
int  cpd_index_weights_from_loads(cpd_index* ix, const uint32_t* capacity /* m, edge order, >= 1 */,
                                  const cpd_vdf* f, cpd_vdf_info* info);
/* The index's current weights in original edge order (m values): what
 * cpd_index_set_weights was given or cpd_index_weights_from_loads wrote, the
 * free-flow weights when no custom weights are set.  Permuted from slot order
 * on the GPU and copied out once, as cpd_query_loads_fetch does.  With
 * parallel edges told apart, as everywhere in this header.                   */
int  cpd_index_get_weights(cpd_index* ix, uint32_t* w /* m, edge order */);
/* The loaded weight sets: *nsets, and when w != NULL set j at w[j * m + e]
 * (*nsets * m values; call with w == NULL first to size it).                */
int  cpd_index_get_weight_sets(cpd_index* ix, uint32_t* nsets, uint32_t* w /* nsets * m, may be NULL */);

/* The method of successive averages over the queries of the last
 * cpd_query_prepare.  Iteration k = 1 .. iters:
 *   1. cpd_query_search_loads(opts, prefix_bytes, demand, k == 1 ? 0 :
 *      CPD_LOADS_ACCUMULATE): an all-or-nothing loading under the current
 *      weights w_k, summed into the resident table;
 *   2. sptt_k = sum over the queries with finished == 1 of demand[q] *
 *      cost[q] (128 bits), the cost being the one found under w_k;
 *   3. cpd_index_weights_from_loads with load_div = k (f->load_div is
 *      ignored): x_k = the mean of the k loadings, w_{k+1} from it, and
 *      tstt_k = x_k . w_{k+1}.
 * Iteration 1 searches under the index's current weights (a caller can warm
 * start); the update after the last iteration is still made, so the index
 * ends with w_{iters+1}.  The relative gap of step k is formed by the CALLER
 * from record k's tstt and record k+1's sptt — (tstt_k - sptt_{k+1}) /
 * tstt_k, both under w_{k+1}; the last record has no such partner.
 * Afterwards cpd_query_fetch and cpd_query_search_counters return the last
 * iteration's search and cpd_query_loads_fetch the summed table (iters times
 * the mean).  The prefix pool's CPD_E_OOM of cpd_query_search_loads passes
 * through from iteration 1 with nothing changed; in a later iteration the
 * call stops there — the message names the iteration — with the table and
 * weights of the iterations that completed (their records are filled, the
 * others zero).  The empty batch is answered: all-zero records, a zeroed
 * table, w0 on every edge.  opts->time_ns without virtual_tick_ns is a wall
 * clock limit, honoured as cpd_query_search honours it: such a loop is not
 * reproducible.  CPD_E_ARG for iters outside 1..65535, a NULL out or
 * capacity, a capacity of 0, f out of range, an incomplete index.
 * Out of scope: a demand set larger than one prepared batch (write the loop
 * from cpd_query_search_loads(CPD_LOADS_ACCUMULATE) and
 * cpd_index_weights_from_loads(load_div), which is why both are public); a
 * time-dependent search.  (The line search step is cpd_query_assign_line
 * below, the conjugate step cpd_query_assign_conj, the bi-conjugate step
 * cpd_query_assign_bi.)                                                      */
typedef struct cpd_assign_iter {
    uint64_t finished;          /* queries with finished == 1 in this iteration  */
    uint64_t sptt_lo, sptt_hi;  /* sum over those of demand[q] * cost[q], under the weights searched with */
    uint64_t tstt_lo, tstt_hi;  /* this iteration's cpd_vdf_info sum: x_k . w_{k+1} */
    uint64_t moves, changed;    /* counter adds of the loading; edges with w_{k+1} != w0 */
    double   search_ms, loads_ms, vdf_ms;
} cpd_assign_iter;
int  cpd_query_assign(cpd_index* ix, const cpd_search_opts* opts, uint64_t prefix_bytes,
                      const uint32_t* demand /* nq, caller order; NULL = 1 each */,
                      const uint32_t* capacity /* m, edge order, >= 1 */,
                      const cpd_vdf* f /* load_div ignored */, uint32_t iters /* 1..65535 */,
                      cpd_assign_iter* out /* iters records */);

/* The flow step — a line search (the Frank-Wolfe step rule) in place of
 * MSA's 1/k.  A FLOW TABLE is state of the index of its own: one u64 X per
 * adjacency slot, in the load table's slot order, the volume in Q16 (x = X >>
 * 16).  It is independent of the load table (cpd_query_loads_clear leaves it
 * alone), lives until cpd_index_flow_clear or cpd_index_free, and is carved
 * from the arena as the load table is.  Let Y be the resident ONE-PLANE load
 * table (cpd_query_loads with nslices = 1, cpd_query_search_loads): the
 * all-or-nothing loading to step towards.  For a slot holding a real edge with
 * free-flow weight w0 and capacity c:
 *     D      = (Y << 16) - X                     signed
 *     X(l)   = X + floor(l * D / 2^16)           l = lambda in 0..65536; the
 *                                                product is formed exactly (it
 *                                                can need 80 bits), the floor
 *                                                is toward minus infinity
 *     w(l)   = the delay function above at x = X(l) >> 16, load_div = 1
 *     g(l)   = sum over the slots of D * w(l)    signed 128 bits, exact
 * X(0) = X, X(65536) = Y << 16, and X(l) stays between them.  Every counter of
 * Y must be below 2^47 (so that Y << 16 < 2^63): CPD_E_RANGE otherwise, naming
 * the first offending edge, with nothing changed.  |D * w| < 2^95 over fewer
 * than 2^32 slots, so g fits; integer adds commute, so every value is exact
 * and the same in every run.
 * The line rule (lambda_q16 == CPD_STEP_LINE), a procedure, so that truncation
 * in g cannot make two implementations disagree:
 *   1. g(0) >= 0: lambda = 0;
 *   2. else g(65536) < 0: lambda = 65536;
 *   3. else lo = 0, hi = 65536; while hi - lo > 1: mid = (lo + hi) >> 1; g(mid)
 *      < 0 ? lo = mid : hi = mid; then lambda = hi.
 * At most 18 evaluations of g.  An explicit lambda_q16 in 0..65536 skips the
 * rule; g(0) alone is then evaluated, for the report.  The evaluations and the
 * decisions between them all run on the device, queued at once: the host reads
 * the outcome once, after the apply pass.
 * Apply: X <- X(lambda); the index's CURRENT weights become w(lambda) on every
 * real edge — the state cpd_index_set_weights(w') leaves (padding slots are
 * copied unchanged; the search's incumbent tables are rebuilt at the next
 * search, as after cpd_index_weights_from_loads); cpd_index_set_weights(ix,
 * NULL) still restores free flow and leaves the flow table as it is.
 * No flow table resident: the step initialises X = Y << 16 whatever lambda_q16
 * says and reports lambda = 65536, evals = 0, g0 = 0, xw0 = 0 (from X = 0
 * every D is >= 0 and the rule would answer 0).
 * The exact relative gap before a step is -g0 / xw0 — total time on the
 * current flow minus the time of the all-or-nothing loading, over the former,
 * both under the current flow's weights: the caller forms it from ONE record.
 * CPD_E_ARG, naming the value: no resident load table, or a sliced or timed
 * one; an incomplete index; capacity NULL or some capacity 0; f out of range
 * (load_div is ignored); lambda_q16 in 65537..0xFFFFFFFE; cpd_index_flow_fetch
 * without a resident flow table.  On every error the flow table, the weights
 * and the load table are untouched.
 * cpd_index_flow_fetch: X in original edge order (m values, Q16), permuted on
 * the GPU and copied out once.  cpd_index_flow_clear drops the table.         */
#define CPD_STEP_LINE 0xFFFFFFFFu
typedef struct cpd_flow_info {
    uint32_t lambda_q16;        /* the step taken */
    uint32_t evals;             /* evaluations of g made */
    uint64_t g0_lo, g0_hi;      /* g(0), signed 128: minus the gap's numerator, Q16 */
    uint64_t xw0_lo, xw0_hi;    /* sum of X * w(0), unsigned 128, Q16: the gap's denominator */
    uint64_t tstt_lo, tstt_hi;  /* after the step: sum of (X >> 16) * w', as cpd_vdf_info */
    uint64_t changed;           /* edges with w' != w0 */
    double   line_ms, apply_ms; /* device time of the evaluations / of the apply pass */
} cpd_flow_info;
int  cpd_index_flow_step(cpd_index* ix, const uint32_t* capacity /* m, edge order, >= 1 */,
                         const cpd_vdf* f /* load_div ignored */,
                         uint32_t lambda_q16 /* 0..65536 or CPD_STEP_LINE */,
                         cpd_flow_info* info /* may be NULL */);
int  cpd_index_flow_fetch(cpd_index* ix, uint64_t* flow /* m, edge order, Q16 */);
int  cpd_index_flow_clear(cpd_index* ix);

/* cpd_query_assign with the line rule.  The flow table is cleared first (once
 * the first loading has succeeded: an error of iteration 1 changes nothing).
 * Iteration k = 1 .. iters:
 *   1. cpd_query_search_loads(opts, prefix_bytes, demand, 0): a fresh
 *      all-or-nothing loading Y under the current weights (iteration 1: the
 *      weights the index holds, so a warm start works as in cpd_query_assign);
 *   2. sptt_k as cpd_query_assign forms it;
 *   3. cpd_index_flow_step(CPD_STEP_LINE): iteration 1 initialises X = Y << 16.
 * The loop stops early after an iteration k >= 2 whose lambda is 0: the
 * weights are unchanged, and a deterministic search would find the same
 * routes and the same lambda again (this holds only without a wall-clock
 * opts->time_ns).  *done = the records filled; the rest are zero.  The
 * capacities are uploaded once.  Record k's -g0 / xw0 is the exact relative
 * gap BEFORE step k; no partner record is needed.  Afterwards cpd_query_fetch
 * and cpd_query_search_counters return the last iteration's search,
 * cpd_query_loads_fetch its loading, cpd_index_flow_fetch the flow.  The
 * prefix pool's CPD_E_OOM and the flow step's CPD_E_RANGE pass through from
 * iteration 1 with nothing changed; in a later iteration the call stops there,
 * the message naming the iteration, with the flow table and weights of the
 * iterations that completed.  The empty batch is answered: the flow table
 * zeroed, w0 on every edge, *done = 1 and that record's counts all zero apart
 * from lambda_q16 = 65536, what the initialising step reports.  CPD_E_ARG as
 * cpd_query_assign, and for a NULL done.                                     */
typedef struct cpd_assign_line_iter {
    uint64_t finished;          /* as cpd_assign_iter */
    uint64_t sptt_lo, sptt_hi;
    uint64_t tstt_lo, tstt_hi;  /* cpd_flow_info's: the flow after the step under its weights */
    uint64_t moves, changed;
    double   search_ms, loads_ms, vdf_ms;  /* vdf_ms: the apply pass (+ the capacity upload in record 1) */
    uint32_t lambda_q16, evals; /* as cpd_flow_info */
    uint64_t g0_lo, g0_hi;
    uint64_t xw0_lo, xw0_hi;
    double   line_ms;
} cpd_assign_line_iter;
int  cpd_query_assign_line(cpd_index* ix, const cpd_search_opts* opts, uint64_t prefix_bytes,
                           const uint32_t* demand /* nq, caller order; NULL = 1 each */,
                           const uint32_t* capacity /* m, edge order, >= 1 */,
                           const cpd_vdf* f /* load_div ignored */, uint32_t iters /* 1..65535 */,
                           cpd_assign_line_iter* out /* iters records */,
                           uint32_t* done /* records filled */);

/* The conjugate step — the flow step towards a TARGET other than the new
 * loading: a convex combination of the previous target and the new
 * all-or-nothing loading, chosen conjugate to the previous direction under the
 * Hessian of the objective (Mitradjieva and Lindberg's conjugate Frank-Wolfe).
 * A plain Frank-Wolfe direction zig-zags; this costs two more slot-wise passes
 * per step and no extra search.  A TARGET TABLE S is state of the index beside
 * the flow table: one u64 per adjacency slot, Q16, in the flow table's order —
 * the point the last step aimed at — carved from the arena as the flow table
 * is.  It exists only after the calls of this section; cpd_index_flow_clear
 * drops it with the flow table, and cpd_index_flow_step drops it too, since it
 * moves X without knowing S.  cpd_query_loads_clear and cpd_index_set_weights
 * leave it alone.
 * A procedure, so that two implementations cannot disagree.  For a slot
 * holding a real edge let Y be the resident one-plane load table and Yq = Y <<
 * 16, X the flow and S the target; with no target table resident S is taken to
 * be X.  w0, c and the delay function's parameters are as in the flow step.
 * Range.  Every counter of Y must be below 2^30: CPD_E_RANGE otherwise, naming
 * the first offending edge, with nothing changed.  Tighter than the flow
 * step's 2^47, so that the sums below provably fit: when X and S were made by
 * conjugate steps alone, |db|, |df| <= 2^30.
 * The slope h of the delay function at x = X >> 16, Q16 per unit volume,
 * saturating:
 *     r   as in the delay function (Q16, clamped at 16.0)
 *     q   = (power == 1) ? 1 << 16 : r;
 *           repeat power - 2 times:  q = (q * r) >> 16              q <= 2^28
 *     t   = (w0 * q) >> 16                                          t <  2^44
 *     u   = (t * a_num * power) / a_den                       product <  2^62
 *     h   = (u >= ((u64)c << 16)) ? 0xFFFFFFFF : (u << 16) / c
 * All divisions truncate.  The clamp of r is ignored on purpose: the slope of
 * the clamped function is 0 there, which would switch the conjugacy off
 * exactly where congestion is worst.
 * The sums, one pass over the slots:
 *     db  = (S - X) >> 16        arithmetic shift: the floor, for negative
 *     df  = (Yq - X) >> 16       values too
 *     N   = sum of db * df * h           signed 128
 *     M   = sum of db * db * h           unsigned 128
 *     gy  = sum of (Yq - X) * w(0)       signed 128: minus the gap's numerator
 *     xw0 = sum of X * w(0)              as the flow step
 * Each term of N or M is below 2^92 in magnitude; fewer than 2^32 slots give
 * less than 2^124, and N - M fits signed 128 bits.  Slots with db == 0 add
 * nothing to N and M and skip h.  (After plain flow steps over larger counters
 * the differences can be larger; the sums are then taken mod 2^128.)
 * alpha (alpha_q16 == CPD_ALPHA_CONJ), with Dn = N - M:
 *     Dn == 0, or N == 0, or N and Dn of opposite sign:   alpha = 0
 *     else a = (|N| >= |Dn|) ? CPD_ALPHA_MAX : floor(|N| * 65536 / |Dn|)
 *          alpha = min(a, CPD_ALPHA_MAX)
 * CPD_ALPHA_MAX is 0.99 in Q16: the target never collapses onto the old one.
 * An explicit alpha_q16 in 0..CPD_ALPHA_MAX skips the rule; the sums are still
 * made and reported.  The division is 16 shift-and-subtract steps on 128-bit
 * magnitudes in one lane of the device: |N| < |Dn| < 2^127 there, so the
 * doubled remainder fits.
 * New target.  S <- Yq + floor(alpha * (S - Yq) / 2^16), the product formed
 * exactly and the floor toward minus infinity as in X(l).  alpha = 0 gives S =
 * Yq, whatever S was.
 * Line search and apply.  Exactly the flow step's with D = S - X (the new S) in
 * place of (Y << 16) - X: the same line rule, an explicit lambda_q16 in
 * 0..65536 or CPD_STEP_LINE; then X <- X(lambda), the current weights become
 * w(lambda), tstt and changed are reported as there.  With alpha = 0 every
 * value the step reports and writes equals what cpd_index_flow_step reports
 * and writes from the same state, bit for bit, and gy == g0.
 * No flow table resident: X and S are both initialised to Yq; the step reports
 * alpha 0, lambda 65536, evals 0 and all sums 0.
 * The sums, the alpha decision, the target pass, the 18 evaluate / decide pairs
 * and the apply pass are queued at once; the host reads the outcome once.  The
 * target pass writes S only after the decision has accepted the range.
 * The exact relative gap before the step is -gy / xw0, from ONE record; g0 is
 * g(0) along S - X and no longer the gap's numerator.
 * CPD_E_ARG as the flow step, and for alpha_q16 in CPD_ALPHA_MAX + 1 ..
 * 0xFFFFFFFE; cpd_index_target_fetch without a resident target table.  On
 * every error X, S, the weights and the load table are untouched.
 * cpd_index_target_fetch: S in original edge order, as cpd_index_flow_fetch
 * reads X.                                                                   */
#define CPD_ALPHA_CONJ 0xFFFFFFFFu
#define CPD_ALPHA_MAX  64881u
typedef struct cpd_conj_info {
    uint32_t alpha_q16;         /* the alpha taken */
    uint32_t lambda_q16;        /* the step taken */
    uint32_t evals;             /* evaluations of g made */
    uint64_t n_lo, n_hi;        /* N, signed 128 */
    uint64_t m_lo, m_hi;        /* M, unsigned 128 */
    uint64_t gy_lo, gy_hi;      /* gy, signed 128: minus the gap's numerator, Q16 */
    uint64_t xw0_lo, xw0_hi;    /* sum of X * w(0), unsigned 128, Q16: the gap's denominator */
    uint64_t g0_lo, g0_hi;      /* g(0) along S - X, after S is updated, signed 128 */
    uint64_t tstt_lo, tstt_hi;  /* after the step: sum of (X >> 16) * w', as cpd_vdf_info */
    uint64_t changed;           /* edges with w' != w0 */
    double   conj_ms, line_ms, apply_ms; /* device time of the sums, decision and target pass /
                                            of the evaluations / of the apply pass */
} cpd_conj_info;
int  cpd_index_flow_step_conj(cpd_index* ix, const uint32_t* capacity /* m, edge order, >= 1 */,
                              const cpd_vdf* f /* load_div ignored */,
                              uint32_t alpha_q16 /* 0..CPD_ALPHA_MAX or CPD_ALPHA_CONJ */,
                              uint32_t lambda_q16 /* 0..65536 or CPD_STEP_LINE */,
                              cpd_conj_info* info /* may be NULL */);
int  cpd_index_target_fetch(cpd_index* ix, uint64_t* s /* m, edge order, Q16 */);

/* cpd_query_assign_line with the conjugate step.  The flow and target tables
 * are cleared first (once the first loading has succeeded).  Iteration k makes
 * a fresh loading, forms sptt_k and runs cpd_index_flow_step_conj with
 * CPD_STEP_LINE and alpha = CPD_ALPHA_CONJ, with one exception: after a record
 * with lambda == 0 and alpha > 0 the conjugate direction went nowhere, and the
 * next iteration passes alpha = 0 — a restart with a plain Frank-Wolfe step.
 * The loop stops early after an iteration k >= 2 with lambda == 0 and alpha ==
 * 0.  Error pass-through, the empty batch and *done are as
 * cpd_query_assign_line; record k's -gy / xw0 is the exact relative gap before
 * step k.  Afterwards cpd_index_target_fetch returns the last target.  A
 * record is cpd_assign_line_iter's fields followed by alpha, n, m and gy.    */
typedef struct cpd_assign_conj_iter {
    uint64_t finished;          /* as cpd_assign_line_iter */
    uint64_t sptt_lo, sptt_hi;
    uint64_t tstt_lo, tstt_hi;
    uint64_t moves, changed;
    double   search_ms, loads_ms, vdf_ms;
    uint32_t lambda_q16, evals;
    uint64_t g0_lo, g0_hi;      /* as cpd_conj_info: along S - X */
    uint64_t xw0_lo, xw0_hi;
    double   line_ms;           /* the evaluations and the conjugate passes before them */
    uint32_t alpha_q16;         /* as cpd_conj_info */
    uint64_t n_lo, n_hi;
    uint64_t m_lo, m_hi;
    uint64_t gy_lo, gy_hi;
} cpd_assign_conj_iter;
int  cpd_query_assign_conj(cpd_index* ix, const cpd_search_opts* opts, uint64_t prefix_bytes,
                           const uint32_t* demand /* nq, caller order; NULL = 1 each */,
                           const uint32_t* capacity /* m, edge order, >= 1 */,
                           const cpd_vdf* f /* load_div ignored */, uint32_t iters /* 1..65535 */,
                           cpd_assign_conj_iter* out /* iters records */,
                           uint32_t* done /* records filled */);

/* The bi-conjugate step — the conjugate step with TWO remembered targets: the
 * new target is a convex combination of the new all-or-nothing loading and the
 * last two targets, chosen conjugate to the last two directions (Mitradjieva
 * and Lindberg's bi-conjugate Frank-Wolfe; the conjugate step still zig-zags
 * once two directions alternate).  It costs one more table and a wider sums
 * pass per step, and no extra search.
 * State.  Beside the flow table X and the target table S1 (the conjugate
 * step's S, what cpd_index_target_fetch returns) a SECOND TARGET TABLE S2: one
 * u64 per adjacency slot, Q16, in the flow table's order, carved from the
 * arena as the others are — the target before S1.  The index also keeps
 * lambda_prev, the lambda_q16 of the last step made through this call.  S2
 * exists only after the calls of this section.  cpd_index_flow_clear,
 * cpd_index_flow_step and cpd_index_flow_step_conj drop S2 (they move X or S1
 * without knowing it) and nothing else about them changes;
 * cpd_query_loads_clear and cpd_index_set_weights leave it alone.  Whenever S2
 * is not resident lambda_prev is 65536.
 * A procedure, so that two implementations cannot disagree.  Y is the resident
 * one-plane load table and Yq = Y << 16.  Every counter of Y must be below
 * 2^30: CPD_E_RANGE otherwise, naming the first offending edge, with nothing
 * changed, exactly as the conjugate step refuses.  w0, c, the delay function
 * and the slope h at x = X >> 16 are the conjugate step's, line for line.
 * The step takes one of three branches, reported in info->branch:
 * Branch 0 — no flow table resident.  X = S1 = Yq and S2 is not made; the step
 * reports lambda 65536, evals 0 and every sum, mu, nu, beta and alpha as 0;
 * lambda_prev = 65536.  mu_q16 and nu_q16 are ignored once in range.
 * Branch 1 — S2 not resident, or lambda_prev == 65536: either way there is no
 * usable second direction.  The step is the conjugate step, literally: the
 * same sums N, M, gy and xw0, the same alpha rule when nu_q16 is CPD_BI_AUTO,
 * the same target pass, line search and apply.  Every value it writes to X, S1
 * and the weights and every value it reports equals what
 * cpd_index_flow_step_conj(CPD_ALPHA_CONJ, lambda_q16) writes and reports from
 * the same state, bit for bit.  Then S2 takes the S the alpha rule read: the
 * old S1, or X (before the step) when no target table was resident.  Reported:
 * alpha_q16, a1 = N, b1 = M, beta0 = 65536 - alpha, beta1 = alpha, beta2 = 0,
 * mu = nu = 0, a2 = b2 = 0.  An explicit mu_q16 is ignored here.  An explicit
 * nu_q16 of 0 means alpha = 0, a plain Frank-Wolfe step; any other explicit
 * nu_q16 is CPD_E_ARG in this branch, naming it.
 * Branch 2 — otherwise.  Let lp = lambda_prev (below 65536 here).  Per real
 * slot, every shift arithmetic (a floor):
 *     d1  = (S1 - X) >> 16
 *     d2  = (lp * S1 + (65536 - lp) * S2 - 65536 * X) >> 32
 *     df  = (Yq - X) >> 16
 *     e21 = (S2 - S1) >> 16
 * Tables made by steps of this family alone hold values below 2^46: the
 * bracket in d2 is then below 2^63 in magnitude and every difference below
 * 2^30.  (After plain flow steps over larger counters the expressions are
 * taken mod 2^64 and the sums mod 2^128.)  The sums, one pass over the slots:
 *     A1  = sum of d1 * df  * h          signed 128
 *     B1  = sum of d1 * d1  * h          unsigned 128
 *     A2  = sum of d2 * df  * h          signed 128
 *     B2  = sum of d2 * e21 * h          signed 128
 *     gy  = sum of (Yq - X) * w(0)       as the conjugate step
 *     xw0 = sum of X * w(0)
 * Each term of A1, B1, A2, B2 is below 2^92 in magnitude, fewer than 2^32
 * slots give less than 2^124.  A slot with d1 == 0 and d2 == 0 skips h.
 * Then one lane decides; quotients are mathematical integers, saturated at
 * CPD_BI_MAX = 2^23 - 1 (just under 128.0 in Q16):
 *     mu  = (A2 == 0 or B2 == 0 or A2, B2 of the same sign) ? 0
 *           : min(floor(|A2| * 65536 / |B2|), CPD_BI_MAX)
 *                                             unless mu_q16 is explicit
 *     nu1 = (B1 == 0 or A1 >= 0) ? 0 : min(floor(|A1| * 65536 / B1), CPD_BI_MAX)
 *     nu  = min(nu1 + floor(mu * lp / (65536 - lp)), CPD_BI_MAX)
 *                                             unless nu_q16 is explicit
 *     beta0 = floor(2^32 / (65536 + mu + nu))
 *     beta2 = (mu * beta0) >> 16
 *     beta1 = 65536 - beta0 - beta2
 * This is mu = -d2'H dFW / d2'H (s2 - s1) and nu = -d1'H dFW / d1'H d1 + mu
 * lambda / (1 - lambda) of the paper (d1, d2 the two remembered directions, H
 * the Hessian's diagonal, dFW = y - x), clamped at 0 from below.  beta1 is
 * never negative: beta0 + beta2 <= beta0 * (65536 + mu) / 65536 <= 2^32 *
 * (65536 + mu) / ((65536 + mu + nu) * 65536) <= 65536.  The quotients are made
 * by shift and subtract on 128-bit magnitudes in one lane of the device,
 * integer part (up to 23 bits) and 16 fraction bits: the remainder stays below
 * the divisor, below 2^124, so the doubled remainder fits.
 * New target.  T = floor((beta0 * Yq + beta1 * S1 + beta2 * S2) / 65536), the
 * sum formed exactly; then S2 <- S1 and S1 <- T, per slot, in place.  mu = nu
 * = 0 gives T = Yq.  alpha_q16 is reported as 0.
 * Line search and apply (branches 1 and 2).  Exactly the flow step's with D =
 * S1 - X (the new S1), as in the conjugate step.
 * After every branch lambda_prev becomes the lambda taken.
 * Everything is queued at once and the host reads the outcome once; the range
 * refusal is decided on the device before the target pass writes.
 * The exact relative gap before the step is -gy / xw0, from ONE record.
 * CPD_E_ARG as the conjugate step, and for mu_q16 or nu_q16 in CPD_BI_MAX + 1
 * .. 0xFFFFFFFE (whatever the branch); cpd_index_target2_fetch without a
 * resident S2.  On every error X, S1, S2, lambda_prev, the weights and the
 * load table are untouched.
 * cpd_index_target2_fetch: S2 in original edge order, as cpd_index_flow_fetch
 * reads X.                                                                   */
#define CPD_BI_AUTO 0xFFFFFFFFu
#define CPD_BI_MAX  8388607u
typedef struct cpd_bi_info {
    uint32_t branch;            /* 0, 1 or 2 */
    uint32_t mu_q16, nu_q16;    /* the mu and nu taken (0 in branches 0 and 1) */
    uint32_t beta0_q16, beta1_q16, beta2_q16; /* weights of Yq, S1 and S2 in the new target */
    uint32_t alpha_q16;         /* branch 1: the conjugate step's alpha; else 0 */
    uint32_t lambda_prev_q16;   /* lambda_prev as the step read it */
    uint32_t lambda_q16;        /* the step taken */
    uint32_t evals;             /* evaluations of g made */
    uint64_t a1_lo, a1_hi;      /* A1, signed 128 (branch 1: N) */
    uint64_t b1_lo, b1_hi;      /* B1, unsigned 128 (branch 1: M) */
    uint64_t a2_lo, a2_hi;      /* A2, signed 128 */
    uint64_t b2_lo, b2_hi;      /* B2, signed 128 */
    uint64_t gy_lo, gy_hi;      /* gy, signed 128: minus the gap's numerator, Q16 */
    uint64_t xw0_lo, xw0_hi;    /* sum of X * w(0), unsigned 128, Q16: the gap's denominator */
    uint64_t g0_lo, g0_hi;      /* g(0) along S1 - X, after S1 is updated, signed 128 */
    uint64_t tstt_lo, tstt_hi;  /* after the step: sum of (X >> 16) * w', as cpd_vdf_info */
    uint64_t changed;           /* edges with w' != w0 */
    double   bi_ms, line_ms, apply_ms; /* device time of the sums, decision and target pass /
                                          of the evaluations / of the apply pass */
} cpd_bi_info;
int  cpd_index_flow_step_bi(cpd_index* ix, const uint32_t* capacity /* m, edge order, >= 1 */,
                            const cpd_vdf* f /* load_div ignored */,
                            uint32_t mu_q16 /* 0..CPD_BI_MAX or CPD_BI_AUTO */,
                            uint32_t nu_q16 /* 0..CPD_BI_MAX or CPD_BI_AUTO */,
                            uint32_t lambda_q16 /* 0..65536 or CPD_STEP_LINE */,
                            cpd_bi_info* info /* may be NULL */);
int  cpd_index_target2_fetch(cpd_index* ix, uint64_t* s2 /* m, edge order, Q16 */);

/* cpd_query_assign_conj with the bi-conjugate step.  The flow table and both
 * target tables are cleared first (once the first loading has succeeded).
 * Iteration k makes a fresh loading, forms sptt_k and runs
 * cpd_index_flow_step_bi with CPD_STEP_LINE and mu = nu = CPD_BI_AUTO, with
 * one exception: after a record with lambda == 0 and (mu > 0 or nu > 0 or
 * alpha > 0) the direction went nowhere, and the next iteration passes mu = nu
 * = 0 — a restart with a plain Frank-Wolfe step.  The loop stops early after
 * an iteration k >= 2 with lambda == 0 and mu == nu == alpha == 0.  Error
 * pass-through, the empty batch and *done are as cpd_query_assign_conj; record
 * k's -gy / xw0 is the exact relative gap before step k.  Afterwards
 * cpd_index_target_fetch and cpd_index_target2_fetch return the last two
 * targets.  A record is cpd_assign_line_iter's fields followed by branch, mu,
 * nu, beta0..2, alpha, a1, b1, a2, b2 and gy.                                */
typedef struct cpd_assign_bi_iter {
    uint64_t finished;          /* as cpd_assign_line_iter */
    uint64_t sptt_lo, sptt_hi;
    uint64_t tstt_lo, tstt_hi;
    uint64_t moves, changed;
    double   search_ms, loads_ms, vdf_ms;
    uint32_t lambda_q16, evals;
    uint64_t g0_lo, g0_hi;      /* as cpd_bi_info: along S1 - X */
    uint64_t xw0_lo, xw0_hi;
    double   line_ms;           /* the evaluations and the bi-conjugate passes before them */
    uint32_t branch, mu_q16, nu_q16;   /* as cpd_bi_info */
    uint32_t beta0_q16, beta1_q16, beta2_q16;
    uint32_t alpha_q16;
    uint64_t a1_lo, a1_hi;
    uint64_t b1_lo, b1_hi;
    uint64_t a2_lo, a2_hi;
    uint64_t b2_lo, b2_hi;
    uint64_t gy_lo, gy_hi;
} cpd_assign_bi_iter;
int  cpd_query_assign_bi(cpd_index* ix, const cpd_search_opts* opts, uint64_t prefix_bytes,
                         const uint32_t* demand /* nq, caller order; NULL = 1 each */,
                         const uint32_t* capacity /* m, edge order, >= 1 */,
                         const cpd_vdf* f /* load_div ignored */, uint32_t iters /* 1..65535 */,
                         cpd_assign_bi_iter* out /* iters records */,
                         uint32_t* done /* records filled */);

/* ------------------------------------------------------------------------ */
/* [gpu] Per-kernel device timing (HIP events on the library's stream).      */
typedef struct cpd_kernel_time {
    char     name[32];
    uint64_t launches;
    double   ms;            /* summed device time                            */
    double   bytes;         /* summed algorithmic bytes      */
} cpd_kernel_time;

int  cpd_timing_enable(cpd_graph* g, int enable);
int  cpd_timing_reset(cpd_graph* g);
/* Fills up to `max` entries, returns the number in *count. */
int  cpd_timing_get(const cpd_graph* g, cpd_kernel_time* out, int max,
                    int* count);

#ifdef __cplusplus
}
#endif
#endif /* CPD_API_H */
