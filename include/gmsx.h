/* gmsx.h — C-ABI of the MI355X-native set-intersection / subgraph-enumeration backend for GMS.
 *
 * Plain C: opaque handles, raw pointers and sizes, int status codes.  No exceptions, no exit(),
 * no torch / STL types cross this boundary.  This is the boundary a GMS maintainer binds to; the
 * C++ adaptor that plugs it under the reference's template concept is include/gmsx_set_graph.hpp
 * and the reference-side glue is shown in INTEGRATION.md.
 *
 * Every entry point names the reference interface it replaces (paths relative to the spcl/gms
 * tree, i.e. /root/reference).
 *
 * Conventions
 *   - status: 0 = GMSX_OK, negative = error (gmsx_strerror()).  Outputs are written only on success.
 *   - host buffers stay caller-owned; the library copies what it keeps.
 *   - graphs are symmetric CSR: int64 offsets[n+1], int32 neigh[offsets[n]], each row sorted
 *     ascending, duplicate- and loop-free (exactly what the reference loader yields,
 *     gms/third_party/gapbs/builder.h:206-235); gmsx_csr_* builds such graphs, and
 *     gmsx_graph_upload() verifies the invariant on the device unless told not to.
 *   - one device per process (one process per GPU); handles are immutable after creation and may be
 *     used from one host thread at a time, like the reference's main-thread kernel invocation
 *     (gms/common/benchmark.h:111-118).
 */
#ifndef GMSX_H
#define GMSX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GMSX_VERSION 320

/* ---- status codes ---- */
enum {
    GMSX_OK = 0,
    GMSX_ERR_INVALID = -1,      /* bad argument (NULL, negative size, k out of range, …) */
    GMSX_ERR_NOMEM = -2,        /* host allocation failed */
    GMSX_ERR_IO = -3,           /* file could not be opened / parsed (reference: exit(-2)/(-6), reader.h:223-229,270-273) */
    GMSX_ERR_FORMAT = -4,       /* unknown suffix or malformed file (reference: exit(-3), reader.h:243-245) */
    GMSX_ERR_DIRECTED = -5,     /* a directed graph where the path needs an undirected one (reference: exit(100), cli/cli.h:166-171) */
    GMSX_ERR_NO_DEVICE = -6,    /* no HIP device / gmsx_init() not called / HIP runtime error */
    GMSX_ERR_DEVICE_MEM = -7,   /* hipMalloc failed */
    GMSX_ERR_NOT_CANONICAL = -8,/* CSR rows not sorted / not loop-free / not symmetric where required */
    GMSX_ERR_OVERFLOW = -9,     /* ids do not fit int32 (reference: exit(-31), generator.h:41-48) */
    GMSX_ERR_UNSUPPORTED = -10, /* valid request outside what this build implements */
    GMSX_ERR_KERNEL = -11,      /* a kernel launch or device synchronisation failed */
    GMSX_ERR_COMM = -12,        /* librccl missing or an RCCL call failed */
    GMSX_ERR_TIMEOUT = -13      /* a peer of the communicator did not arrive within GMSX_COMM_TIMEOUT_S seconds (gmsx_comm_init / gmsx_comm_allreduce_u64) */
};
const char *gmsx_strerror(int status);
int gmsx_version(void);

/* =====================================================================================
 * Host graph substrate  (replaces gms/third_party/gapbs: generator.h, builder.h, reader.h, writer.h)
 * ===================================================================================== */
typedef struct gmsx_csr gmsx_csr; /* host-resident CSR, replaces CSRGraph (gapbs/graph.h:93-374) */

enum { GMSX_GEN_KRONECKER = 0, GMSX_GEN_UNIFORM = 1 }; /* "-g kronecker|uniform" (cli/cli.h:111-114) */
enum {
    GMSX_RELABEL_NEVER = 0,
    GMSX_RELABEL_AUTO = 1,  /* relabel by decreasing degree iff WorthRelabelling (gapbs/benchmark.h:158-176) — what parse_and_load does (cli/cli.h:174-176) */
    GMSX_RELABEL_ALWAYS = 2
};

/* Generator::GenerateEL + Builder::MakeGraph (+ optional RelabelByDegree): bit-identical CSR to the
 * reference's "-g kronecker|uniform <scale> --deg <degree>" (generator.h:64-127, builder.h:1642-1660).
 * threads<=0: OpenMP default.  The output does not depend on the thread count. */
int gmsx_csr_generate(int generator, int scale, int degree, int relabel, int threads, gmsx_csr **out);

/* The same generator/builder pipeline with caller-chosen R-MAT quadrant probabilities (the reference hard-codes
 * A/B/C = .57/.19/.19, generator.h:82; with those values the result equals gmsx_csr_generate(KRONECKER)).  Used to
 * calibrate the skew of the Bron–Kerbosch workload. */
int gmsx_csr_generate_rmat(int scale, int degree, double a, double b, double c, int relabel, int threads, gmsx_csr **out);

/* Builder::MakeGraphFromEL + SquishGraph on a caller-supplied edge list (builder.h:279-298,237-251):
 * num_nodes<0 → max id + 1; symmetrize!=0 inserts both directions (the only mode the hot path accepts).
 * Rows come out sorted, de-duplicated and loop-free. */
int gmsx_csr_from_edges(int64_t num_nodes, int64_t num_edges, const int32_t *src, const int32_t *dst,
                        int symmetrize, int relabel, gmsx_csr **out);

/* Reader::ReadFile / ReadSerializedGraph by suffix (reader.h:220-250): ".el" text pairs (:49-56), ".wel" weighted pairs
 * (:58-66, weights dropped), ".gr" DIMACS (:68-84), ".graph" METIS (:86-142), ".mtx" Matrix Market coordinate (:146-218),
 * ".sg" binary CSR (:252-305); plus ".sgx", this library's mappable cache form of .sg (gmsx_csr_save_sgx).  Other suffixes → GMSX_ERR_FORMAT. */
int gmsx_csr_load(const char *path, int symmetrize, int relabel, gmsx_csr **out);
/* Writer::WriteSerializedGraph (writer.h:39-69). */
int gmsx_csr_save_sg(const gmsx_csr *g, const char *path);
/* The cache form of the same CSR, ".sgx": the .sg arrays behind a 64-byte header, each at a 64-byte aligned file offset (the reference's
 * .sg puts its int64 offsets at byte 17, so it cannot be used in place).  gmsx_csr_load(".sgx") MAPS the file (private, never written back)
 * instead of reading it: the ranks of a multi-GPU run that load one cache share one copy in the page cache — SURVEY §8(e)'s "replicate the
 * CSR" without N private host copies —, after the same validation as .sg (monotone offsets, ids in range).  gmsx_csr_is_mapped: 1 if the
 * handle's arrays are such a mapping. */
int gmsx_csr_save_sgx(const gmsx_csr *g, const char *path);
int gmsx_csr_is_mapped(const gmsx_csr *g);
/* Wrap (copy) caller arrays; validates monotone offsets and id range. */
int gmsx_csr_from_arrays(int64_t n, const int64_t *offsets, const int32_t *neigh, gmsx_csr **out);

/* SourcePicker (gapbs/benchmark.h:51-75): out[0 .. count) = the first `count` picks — mt19937(kRandSeed), uniform over [0, n), redrawn while the
 * degree is 0; given >= 0: `count` copies of it (given >= n → GMSX_ERR_INVALID).  A graph with no edge → GMSX_ERR_INVALID where the reference
 * would draw for ever.  Host only. */
int gmsx_csr_pick_sources(const gmsx_csr *g, int64_t count, int32_t given /* -1: random */, int32_t *out /* count, host */);
int gmsx_csr_worth_relabelling(const gmsx_csr *g);                  /* gapbs/benchmark.h:158-176; 1/0 */
int gmsx_csr_relabel_by_degree(const gmsx_csr *g, gmsx_csr **out);  /* builder.h:1699-1733 */

int64_t gmsx_csr_num_nodes(const gmsx_csr *g);          /* CSRGraph::num_nodes */
int64_t gmsx_csr_num_edges(const gmsx_csr *g);          /* CSRGraph::num_edges  (= nnz/2, graph.h:186) */
int64_t gmsx_csr_num_edges_directed(const gmsx_csr *g); /* nnz */
const int64_t *gmsx_csr_offsets(const gmsx_csr *g);     /* n+1 entries; valid until gmsx_csr_free */
const int32_t *gmsx_csr_neighbors(const gmsx_csr *g);   /* nnz entries */
/* Σ_{(u,v)∈E,u<v}(d_u+d_v): element count behind the algorithmic-bytes figure. */
uint64_t gmsx_csr_merge_elements(const gmsx_csr *g);
/* FNV-1a-64 of the offsets / neighbour arrays (loader fingerprints); 2 = the weight array, 0 for an unweighted CSR. */
uint64_t gmsx_csr_fingerprint(const gmsx_csr *g, int which /*0 offsets, 1 neighbours, 2 weights*/);
void gmsx_csr_free(gmsx_csr *g);

/* ---- EDGE WEIGHTS: a gmsx_csr may own int32 weights[nnz], parallel to its neighbour array (the reference's WGraph = CSRGraph<NodeId,
 * NodeWeight<NodeId, int32>>, gapbs/benchmark.h).  Host only.  Every call above behaves on a weighted CSR exactly as on its structure
 * (gmsx_csr_save_sg / _sgx write the structure only); gmsx_csr_relabel_by_degree carries a weight with its arc (rows re-sorted by id, each
 * weight staying with its id) — where the reference's RelabelByDegree would reset every weight to 1.
 * gmsx_csr_weights: the array (valid until gmsx_csr_free), or NULL for an unweighted CSR.
 * gmsx_csr_generate_weighted: WeightedBuilder::MakeGraph for "-g/-u SCALE -k DEGREE -s" (builder.h:1642-1660): the edge list of
 * gmsx_csr_generate, weights by Generator::InsertWeights (generator.h:131-146) over that list BEFORE symmetrisation — one mt19937 per block of
 * 2^18 edges seeded kRandSeed + block, uniform_int_distribution<int>(1, 255) —, both directions of an edge carry its weight (builder.h:104), a
 * row is sorted by (id, weight) and made unique by id (graph.h:39-46), so a repeated edge keeps its SMALLEST weight; self loops are dropped.  The
 * result is symmetric in structure and in weights, bit-identical to the reference's and independent of the thread count.
 * gmsx_csr_from_weighted_edges: the same builder on a caller's list; w == NULL = InsertWeights over that list (the reference on a weightless .el).
 * gmsx_csr_load_weighted: ".wel", ".gr" and ".wsg" (reader.h:252-305: the neighbour array as {int32 id, int32 weight} pairs) keep their
 * weights (a text weight outside int32 → GMSX_ERR_OVERFLOW; weights below 1 are loaded as they are: gmsx_graph_set_weights refuses them);
 * ".el" gets InsertWeights in file order; ".sg" / ".sgx" → GMSX_ERR_FORMAT (the reference exits with -5); ".mtx" and ".graph" →
 * GMSX_ERR_UNSUPPORTED from this entry point (their readers drop the weight column).
 * gmsx_csr_save_wsg: Writer::WriteSerializedGraph of a weighted graph (writer.h:39-69); an unweighted CSR → GMSX_ERR_INVALID.
 * gmsx_csr_from_arrays_weighted: gmsx_csr_from_arrays plus a copy of weights[nnz]. */
const int32_t *gmsx_csr_weights(const gmsx_csr *g);
int gmsx_csr_generate_weighted(int generator, int scale, int degree, int relabel, int threads, gmsx_csr **out);
int gmsx_csr_from_weighted_edges(int64_t num_nodes, int64_t num_edges, const int32_t *src, const int32_t *dst, const int32_t *w /* or NULL */,
                                 int symmetrize, int relabel, gmsx_csr **out);
int gmsx_csr_load_weighted(const char *path, int symmetrize, int relabel, gmsx_csr **out);
int gmsx_csr_save_wsg(const gmsx_csr *g, const char *path);
int gmsx_csr_from_arrays_weighted(int64_t n, const int64_t *offsets, const int32_t *neigh, const int32_t *weights, gmsx_csr **out);

/* Threads of the host substrate (generator, builder, relabelling: OpenMP, like the reference's loader).  n <= 0 restores
 * the runtime default.  Returns the previous maximum.  Launchers that export OMP_NUM_THREADS=1 to their workers
 * (torch.distributed.run does) would otherwise serialise graph generation: the rank that builds the graph calls this. */
int gmsx_set_host_threads(int n);

/* OPTIONS.  The library reads NO tuning from the environment (the one exception is GMSX_COMM_TIMEOUT_S below): limits, budgets, container
 * forms and diagnostics are set by explicit calls.  Every option changes HOW a result is computed — which kernel variant, how large a
 * chunk, what is printed to stderr — and never the result; the "wrong counts" A/B switches of the kernel sources exist only in
 * development builds (-DGMSX_DEV_HOOKS, tools/ab_lib.sh) and are absent from a library built by `make`.
 * name: one of the names below (without prefix), else GMSX_ERR_INVALID; value: a decimal number as a C string (< 32 characters), NULL = back
 * to the default.  Process-wide; set options before the calls they steer, not concurrently with them.  Names:
 *   diagnostics     TIMING (phase times and bin sizes on stderr), MEM_TRACE (one line per device allocation of a graph), BK_VERBOSE
 *   upload          SORT_CHUNK (vertices per row-sort range), UPLOAD_STAGED (0 = one hipMemcpyAsync per array), INIT_LAZY (1 = pin the staging
 *                   buffers at the first large upload instead of in gmsx_init)
 *   triangle count  TC_MEM_LIMIT_MB (budget of the containers: smaller = several passes), INLINE_LIMIT, TC_INLINE_FIRST, TC_TWO_SIDED,
 *                   TC_DELTA / TC_DELTA_PCT / TC_GAP12 / TC_HYBRID / TC_TAIL_DELTA (which container forms the stream rows may take),
 *                   TC_HOT_WINDOWS / TC_HOT_KB / TC_HOT_MIN (L2-window phases of the hub lists), TC_TEST_MAX_UNITS (pretend the task-list
 *                   fields are this narrow), TC_KEEP_ROWS (keep the per-vertex row descriptors for gmsx_tc_row_histogram), TC_OVERLAP,
 *                   TC_PERSIST, TC_ITEM_WGS (launch shapes), TC_CORE (the dense core, read when the containers are built: the oriented edges
 *                   whose pivot-side endpoint has a rank id below K are counted as one masked bit-GEMM on the matrix cores instead of being
 *                   streamed; -1 = K chosen from the graph, a multiple of 1024 or 0 (the default), 0 = no core, N > 0 = K = N; always clamped
 *                   to min(hub ids, n, 32768)), TC_LIGHT_PACKED (read when the containers are built: 1, the default = the edges between two
 *                   light vertices as packed blocks of ids, streamed and compared by search; 0 = as 32-byte pointer records, gathered and
 *                   compared all-pairs), TC_GATHER (read when the containers are built: R = 0 … 7, default 7 (3, then 0, when the device is short of memory) — a stream row that ends inside
 *                   a 128-byte line leaves the R or fewer 16-byte units behind its last line boundary, and a whole row of R or fewer units,
 *                   to a densely packed gathered row of the receiving pivot, so that the row itself is whole lines; bitset rows never; 0 = no
 *                   gathered rows: the task lists of the layout without them)
 *   k-clique        KC_MAXD (widest pivot of the bit-matrix kernels), KC_SLAB_MB (budget of the global slabs), KC_STREAMS (1 … 4 streams for the bins),
 *                   KC_REVERSE (0 = every member row streamed forward: no reverse rows; like KC_REV_* read when the lists of a graph are built, i.e. at its first k-clique call), KC_REV_MIN (edges a hub
 *                   receiver must get to take them, default 64), KC_REV_FACTOR (10 x how much cheaper in bytes the reverse side must be; default 0: every hub edge whose receiver qualifies),
 *                   KC_REV_TAIL (0 = tail members — rank id >= 65 535 — never hand their row to a receiver), KC_REV_TAIL_MIN (edges a tail receiver must get, default 256),
 *                   KC_TRI (0 = k = 4 keeps rectangular LDS matrices up to d+ = 1024 and the global slab beyond, instead of triangular ones up to 1472),
 *                   KC_MFMA (0 = the k = 4 count of the pivots of d+ > 512 by AND + popcount inside their BUILD kernels instead of on the matrix cores),
 *                   KC_POOL_MB (the pool those pivots' matrices pass through, default min(what the call needs, 6144): smaller = more, shorter chunks)
 *   Bron–Kerbosch   BK_MAXC (widest start vertex of the register-resident search), BK_ARENA_MB, BK_BUDGET / BK_BUDGET0 (nodes before a
 *                   search is re-split), BK_GROUPS, BK_SMALL_P, BK_SMALL_P_GROUPS, BK_RESUME_GRAB, BK_SPLIT_BUILD, BK_TINY_ROOTS,
 *                   BK_TINY_BESIDE (kernel variants)
 *   Bron–Kerbosch listing  BK_LIST_ARENA_MB (budget of the search slabs of one launch: smaller = more launches)
 *   k-clique-star listing  KCSTAR_SLAB_MB (budget of the level-set slabs of one launch: smaller = more launches)
 *   core decomposition     CORE_WG_FRONTIER (largest frontier whose rounds run inside the one-workgroup kernel, default 512 — a first guess, not a
 *                   tuned value; 0 = every round is a kernel boundary; test hook)
 *   graph colouring        COLOR_WG_FRONTIER (the same for the rounds of gmsx_coloring_jp: largest frontier whose rounds run inside its one-workgroup
 *                   kernel, default 512 — a first guess; 0 = every round is a kernel boundary; test hook)
 *   truss decomposition    TRUSS_WG_FRONTIER (the same for the rounds of gmsx_truss_decomposition, whose frontier holds edges: default 0 = every
 *                   round is a kernel boundary, which measured faster than the one-workgroup kernel at every size; test hook)
 *   link prediction        LP_LDS_MAXN (largest n whose per-source bitmaps live in LDS, default and maximum 131072 — a first guess; 0 = every
 *                   bitmap in the workgroup's global slab; test hook), LP_SLAB_MB (budget of the candidates of one chunk: smaller = more chunks;
 *                   test hook)
 *   subgraph matching      SGM_LAUNCH_TASKS (tasks per launch of gmsx_subgraph_match, default 2^24 for a listing and 2^16 with GMSX_SGM_FIRST —
 *                   both first guesses, not tuned values; a small value splits a small graph into many launches; test hook)
 *   connected components   CC_SAMPLE (neighbours of every vertex linked in the first pass of gmsx_connected_components, before the giant component
 *                   is picked and skipped; default 2; 0 = no sampling pass: one pass covers every vertex and neighbour), CC_WAVE_ROW / CC_WG_ROW
 *                   (smallest row that gets a wave / a whole workgroup in the linking kernels, defaults 256 / 4096) — all three first guesses,
 *                   not tuned values; test hooks
 *   4-cycles and motifs    C4_LDS_SPAN (largest counter span of a source, in 32-bit counters, kept in a workgroup's LDS; default and maximum
 *                   8192; 0 = no LDS path), C4_SLAB_MB (budget of the global counter spans, default 1024: a smaller budget = fewer workgroup
 *                   spans and fewer split sources per launch), C4_SPLIT_WEDGES (wedge bound above which a source is walked by many workgroups
 *                   into one span, default 2^18; 1 = every source with a wedge, a huge value = none) — all three first guesses, not tuned
 *                   values; test hooks
 *   breadth-first search   BFS_DIRECTION (0, the default = the reference's direction-optimising rule; 1 = every level top-down; 2 = every level
 *                   after the source's bottom-up), BFS_ALPHA (15) / BFS_BETA (18) (bfs.cc:120-121: bottom-up when scout_count > edges_to_check /
 *                   alpha, and for as long as the awake count does not fall or exceeds n / beta), BFS_BU_PROBE (row entries a single lane probes
 *                   in the bottom-up step before the row goes to a 16-lane group or a wave; default 16, at most 1024), BFS_WG_FRONTIER (as
 *                   CORE_WG_FRONTIER for the top-down rounds, default 512; 0 = every round is a kernel boundary) — all first guesses and test
 *                   hooks; none changes depth, parent, scores or any info field except bottom_up_levels; gmsx_betweenness reads them, too
 *   multi-source BFS       MSBFS_DIRECTION (0, the default = the rule: a level is pushed from the active list when the degree sum of that list is
 *                   at most nnz / MSBFS_ALPHA, else pulled by every vertex that still lacks a source; 1 = every level pushed; 2 = every level
 *                   pulled), MSBFS_ALPHA (default 15 — a first guess, not a tuned value), MSBFS_WORDS (W = 1 or 2: 64-bit words
 *                   per vertex, so a pass advances 64 W sources; 0, the default = 1 for a list of at most 64 sources and 2 for a longer one, as
 *                   measured: DESIGN.md §5.4j) — none changes any output of gmsx_bfs_multi but passes, push_levels and
 *                   pull_levels; test hooks.  Under TIMING every level prints its direction and the two operands of the rule
 *   shortest paths         SSSP_WG_FRONTIER (as CORE_WG_FRONTIER for the relaxation rounds of gmsx_sssp, default 512; 0 = every round is a kernel
 *                   boundary), SSSP_WIDE (1 = 64-bit distance words whatever the weights), SSSP_DELTA_AUTO (the parameter c of the default
 *                   bucket width, delta = max(1, c * mean weight / mean degree); default 16 — measured once, DESIGN.md §5.4l, and still a first guess) — test hooks;
 *                   none changes dist, parent or any info field except delta (SSSP_DELTA_AUTO, with delta = 0), buckets (a fact about
 *                   delta), rounds and relaxations
 *   spanning forest        MSF_WAVE_ROW / MSF_WG_ROW (smallest row that gets a wave / a whole workgroup in the search pass of
 *                   gmsx_min_spanning_forest, defaults 256 / 4096, as CC_WAVE_ROW / CC_WG_ROW), MSF_PRUNE (0, the default = every vertex is searched in every
 *                   round; 1 = a vertex without a crossing arc leaves the live list for good, so that later rounds walk the shrinking border
 *                   only — measured slower on four graphs) — the bin edges are first guesses, not tuned values; test hooks;
 *                   none changes any output of gmsx_min_spanning_forest except gmsx_stats
 *   communities            LP_WAVE_ROW (longest row a lane group evaluates with one entry per lane, default and maximum 64; 0 = no such rows),
 *                   LP_LDS_ROW (longest row whose label table lives in a workgroup's LDS, default 2048, at most LP_LDS_SLOTS; 0 = none),
 *                   LP_LDS_SLOTS (slots of that table, a power of two in 16 … 4096, default 4096 = 48 KB of the 160 KB of a compute unit),
 *                   LP_WG_WORK (consecutive colour classes whose rows hold at most this many entries in all are run by one workgroup in one
 *                   launch, default 4096; 0 = every class in launches of its own), LP_ACTIVE (1, the default = from the second sweep on only
 *                   the vertices a neighbour of which changed are evaluated; 0 = every vertex in every sweep) — the three row bounds are first
 *                   guesses, not tuned values; LP_WG_WORK and LP_ACTIVE were set from a measurement; test hooks; none changes any output of gmsx_label_propagation or gmsx_modularity except
 *                   gmsx_stats
 *   matching               MATCH_WAVE_ROW / MATCH_WG_ROW (smallest row that gets a wave / a whole workgroup in the search pass of
 *                   gmsx_greedy_matching, defaults 256 / 4096, as MSF_WAVE_ROW / MSF_WG_ROW), MATCH_KEEP (1, the default = a live vertex whose
 *                   candidate of the last round is still free keeps it without walking its row; 0 = every live vertex searches its row in
 *                   every round) — the bin edges are first guesses, not tuned values; test hooks; none changes any output
 *                   of gmsx_greedy_matching except gmsx_stats (alg_elements, the arcs examined, is smaller or equal under MATCH_KEEP = 1)
 *   biconnectivity         BCC_WAVE_ROW / BCC_WG_ROW (smallest row that gets a wave / a whole workgroup in the row passes of
 *                   gmsx_biconnected_components, defaults 256 / 4096, as CC_WAVE_ROW / CC_WG_ROW), BCC_WG_FRONTIER (largest frontier of the
 *                   BFS forest that one workgroup takes round after round, default 512, as BFS_WG_FRONTIER; 0 = every round a kernel
 *                   boundary), BCC_WG_LEVEL (consecutive levels of the forest that each hold at most this many vertices are swept by one
 *                   workgroup in one launch, default 1024; 0 = every level a launch of its own) — all four are first guesses, not tuned
 *                   values; test hooks; none changes any output of gmsx_biconnected_components except gmsx_stats */
int gmsx_set_option(const char *name, const char *value);
void gmsx_reset_options(void);                          /* every option back to its default */
int gmsx_option_name(int index, const char **name);     /* enumerates the names: GMSX_ERR_INVALID past the last */

/* =====================================================================================
 * Device side
 * ===================================================================================== */
typedef struct gmsx_graph gmsx_graph; /* device-resident graph; replaces SetGraph<Set> (representations/graphs/set_graph.h:10-233) */

typedef struct gmsx_stats {
    double kernel_ms;          /* HIP-event time of the counting kernels of the last call (on the library's stream) */
    double setup_ms;           /* HIP-event time of per-call setup kernels (memsets, bin prep), not in kernel_ms */
    uint64_t units;            /* work units processed: intersect_count calls (edges) / root vertices */
    uint64_t alg_elements;     /* Σ(d_u+d_v) over the units of this call, 0 if n/a */
    uint64_t probes;           /* TC: id slots the oriented kernels probe (8 per list unit, 14 per byte-delta unit, 4 words per bitset
                                * unit, 4 / 6 per tail unit) — the bit products of the dense core (TC_CORE) are NOT counted; BK: resume rounds;
                                * else 0 */
    int32_t launches;          /* number of kernel launches inside kernel_ms */
    int32_t reserved;
    uint64_t stream_bytes;     /* TC (oriented): algorithmic bytes of THIS formulation per call — every pivot's own containers once, plus
                                  for every oriented edge (u,v) the bytes of N+(v) in the form the kernels read: its stream rows (whole
                                  16-byte units of bitset / 16-bit list / byte-delta for the hub part, 32-bit ids / 16-bit delta for the
                                  tail part) or 4 bytes per inverted gather.  No cache is assumed: the traffic a pass would cause if
                                  nothing were ever re-used on chip.  k-clique: every pivot's own containers once + per member the containers of
                                  N+(v) the BUILD reads (bitset words or 16-bit list, tail ids; one 4-byte gather per pair for d+ <= 32) — or, for a
                                  hub member whose row the receivers' pass produced (round 6, kclique.hip: reverse rows), the 2 i bytes of the pivot's
                                  prefix below it + its 16-byte record + its row of ceil(i/32) words written and read back — + the
                                  slab matrices of pivots wider than 1024, written and read once.  Bron-Kerbosch: per start vertex the oriented
                                  rows of all its neighbours (what the builds walk) + Cadj | XT of the start vertices built in the arena, once
                                  + one Cadj row (c / 32 words) per search-tree node — the operand of cand.intersect(N(q)), tomita.h:51-70.
                                  0 for the other entry points. */
} gmsx_stats;

/* Bind this process to one HIP device.  device<0 → current device.  Calling it again with the same device is a no-op (and makes
 * the device current for the calling host thread); a different device → GMSX_ERR_UNSUPPORTED (one device per process). */
int gmsx_init(int device);
/* Use a caller-owned HIP stream (hipStream_t passed as void*) for all subsequent launches; NULL → library stream. */
int gmsx_set_stream(void *hip_stream);
int gmsx_device_info(char *name, size_t name_len, int *compute_units, int64_t *hbm_bytes);
/* Diagnostics: the rate (GB/s) a read-only in-order stream over a `bytes`-sized buffer (choose it far above the 256 MB Infinity Cache) reaches on
 * the bound device, 16-byte loads, `iterations` sweeps timed with HIP events — the measured ceiling bench.py quotes its roofline fractions
 * against beside the 8 TB/s specification peak.  No reference counterpart. */
int gmsx_hbm_read_probe(int64_t bytes, int iterations, double *gbps);

enum {
    GMSX_UPLOAD_DEFAULT = 0,
    GMSX_UPLOAD_TRUSTED = 1, /* skip the device-side check of the canonical-row invariant.  The check (default): every row strictly
                                ascending, ids in range, no self loops — exact — and the arc set equal to its transpose, decided by two
                                keyed 64-bit multiset hashes of both (keys drawn per process): an asymmetric input passes with
                                probability 2^-128, a symmetric one never fails.  With TRUSTED the caller GUARANTEES the invariant (only
                                out-of-range ids are still refused): on a row with a repeated neighbour, a self loop or a missing reverse
                                arc the counts are undefined — the triangle kernels, for one, maintain a pivot's LDS bitmap by XOR, so a
                                repeated id cancels itself */
    GMSX_UPLOAD_FOR_TC = 2   /* also build the triangle-count containers (stream rows, inline rows, task lists: ~5x the CSR) now, inside the
                                upload — what a triangle-count harness wants in its untimed "GraphExec buildTime" (common/benchmark.h:
                                105-109).  Without it they are built by gmsx_graph_prepare or by the first gmsx_tc_* call, and a k-clique /
                                Bron–Kerbosch user never pays for them (the reference's k-clique harness times its SGraph build,
                                k_clique_count_set_based.h:22) */
    /* bits 8..23 (test hook): if non-zero, the hub-container id range is [0, value) instead of [0, 65535), so that
       small graphs exercise the 32-bit tail containers; results never depend on it */
};
#define GMSX_UPLOAD_HUB_LIMIT(x) ((uint32_t)(x) << 8)
/* SetGraph::FromCGraph (set_graph.h:86-89,152-181): copies the CSR into HBM and builds the device-side
 * set representations (degree-oriented DAG rows; the analogue of the per-row SortedSet / RoaringSet
 * construction, sorted_set.h:64-66 / roaring_set.h:49-54).  Timed by callers as "GraphExec buildTime"
 * like the reference (common/benchmark.h:105-109). */
int gmsx_graph_upload(int64_t n, const int64_t *offsets, const int32_t *neigh, uint32_t flags, gmsx_graph **out);
int gmsx_graph_upload_csr(const gmsx_csr *g, uint32_t flags, gmsx_graph **out);
/* The same for ONE rank of a multi-GPU run: the CSR and the oriented containers are complete on every rank (any row may be
 * streamed; k-clique / Bron-Kerbosch shards of any (part, nparts) still work), but the triangle-count containers — task lists and inline
 * rows, ~4/5 of the device bytes — are built for the pivots of shard `part` of `nparts` only, so their memory and build time shrink with
 * the number of ranks.  gmsx_tc_partial on such a graph accepts exactly (part, nparts) (GMSX_TC_FULL any).  part = 0, nparts = 1 is
 * gmsx_graph_upload. */
int gmsx_graph_upload_shard(int64_t n, const int64_t *offsets, const int32_t *neigh, uint32_t flags, int part, int nparts, gmsx_graph **out);
int gmsx_graph_upload_csr_shard(const gmsx_csr *g, uint32_t flags, int part, int nparts, gmsx_graph **out);
/* Builds optional containers of an uploaded graph ahead of their first use (so that a caller can time or place the cost). */
enum { GMSX_PREPARE_TC = 1 /* the triangle-count containers, see GMSX_UPLOAD_FOR_TC */ };
int gmsx_graph_prepare(gmsx_graph *g, uint32_t what);
/* 0 = the triangle-count containers are not built yet; 1 = they hold every pivot (the normal case); k > 1 = they did not fit the device:
 * 1/k of the pivots is resident at a time and every gmsx_tc_* call walks k passes, rebuilding between them (slower, never refused). */
int gmsx_graph_tc_passes(const gmsx_graph *g);
int gmsx_graph_free(gmsx_graph *g);
int64_t gmsx_graph_num_nodes(const gmsx_graph *g);   /* SetGraph::num_nodes, set_graph.h:115-118 */
int64_t gmsx_graph_num_edges(const gmsx_graph *g);   /* undirected edges m */
int64_t gmsx_graph_device_bytes(const gmsx_graph *g);
int32_t gmsx_graph_max_out_degree(const gmsx_graph *g); /* max d+ of the degree-oriented DAG */

/* ---- triangle counting: gms/algorithms/set_based/triangle_count ---- */
enum {
    GMSX_TC_AUTO = 0,
    GMSX_TC_ORIENTED = 1, /* each edge intersects the degree-oriented rows N+(u) ∩ N+(v): every triangle met once */
    GMSX_TC_FULL = 2      /* the reference's formulation verbatim: every edge u<v intersects the FULL rows, total/3
                             (parallel/total.h:13-23); all m full-row intersect_count calls are executed on the device */
};
/* Par::count_total / Seq::count_total (parallel/total.h:7-24, sequential/total.h:7-23): number of triangles. */
int gmsx_tc_total(const gmsx_graph *g, int algo, uint64_t *triangles, gmsx_stats *stats);
/* Shard `part` of `nparts` (cost-balanced, disjoint, covering): returns the UN-divided partial sum so that
 * Σ_parts partial / gmsx_tc_divisor(algo) = triangles.  This is what each rank computes before the single
 * all-reduce of SURVEY §8(e) (the OpenMP reduction(+:total) of parallel/total.h:12). */
int gmsx_tc_partial(const gmsx_graph *g, int algo, int part, int nparts, uint64_t *partial, gmsx_stats *stats);
int gmsx_tc_divisor(int algo); /* 1 for ORIENTED/AUTO, 3 for FULL */
/* Diagnostics: the algorithmic stream bytes of one oriented pass (gmsx_stats.stream_bytes) split by what is read — out[0..2]: the hub
 * stream rows named by the work items' entries, by form (16-bit list, bitset, byte-delta); out[3..4]: the tail stream rows (32-bit
 * list, 16-bit delta); out[5]: the entries themselves; out[6]: the pivots' own containers, once per work item; out[7]: the part of
 * out[0] + out[3] that is inline rows (ids handed over by light pivots); out[8..10]: the light-pivot kernel — hub rows, tail rows of
 * the far light members it streams, and its own lists + descriptors; out[11..14]: counts — entries, inline entries, work items,
 * members streamed by the light-pivot kernel; out[15]: the dense core (TC_CORE) — per 64 x 64 block the fragment bytes of its 2 x 64 rows
 * and its mask words, no reuse assumed; out[16]: K of the core (0 = none); out[17]: the part of
 * out[0] + out[2] + out[3] + out[4] that is gathered rows (TC_GATHER); out[18]: 128 x the 128-byte lines that the rows named by all entries
 * touch — what the row traffic of the item kernels beyond the L2 should approach; out[19]: non-bitset entries whose row ends inside a
 * line; out[20]: the R the containers were built with — TC_GATHER, or what its default fell back to (7, 3, 0) when the gathered rows did not fit
 * the device or the 32-bit first-unit field of a task entry.  out[0..6] + out[8..10] + out[15] = stream_bytes.
 * 21 values, host. */
int gmsx_tc_stream_breakdown(const gmsx_graph *g, uint64_t *out21);
/* Diagnostics: the stream rows named by the work items' entries as a histogram over row length in 16-byte units — out[(cls*24 +
 * bin)*2] rows, [+1] units; cls 0..4 = hub rows as list / bitset / byte-delta, tail rows as list / delta; bin = 1 … 16 units exactly,
 * then 17-32, 33-64, … 1025+; out[240..243]: entries, inline entries, work items, bytes of the pivots' own containers;
 * out[248..251]: Σ over the oriented edges (u,v) of heavy then light pivots u of the stream units of v's rows and of min(units of
 * u's rows, units of v's rows); out[252]: the same sum for heavy u with u's rows cut at v's id (estimate) — out[248..252] are 0 unless the
 * graph was built with GMSX_TC_KEEP_ROWS=1 (the per-vertex row descriptors they read are freed after the build).  256 values, host. */
int gmsx_tc_row_histogram(const gmsx_graph *g, uint64_t *out256);
/* Diagnostics (round 5, the "stream a row once against several staged pivots" question): if the heavy pivots were processed in batches of
 * `batch` consecutive positions of the d+ order, each distinct stream row of a batch loaded once — out[0] entries of the hub work items,
 * out[1] the 16-byte units they stream per pass today, out[2] distinct (batch, row) pairs, out[3] the units a batched pass would stream
 * (every row once per batch, at the longest cut any pivot of the batch reads), out[4] hub work items.  batch = 1 shows what rows repeat
 * inside one pivot's own list (inline chunks never do).  8 values, host. */
int gmsx_tc_comembership(const gmsx_graph *g, int batch, uint64_t *out8);
/* Par::vertex_count2 / vertex_count2_once (parallel/vertex.h:14-49): counts[u] = Σ_{v∈N(u)} |N(u)∩N(v)| (= 2·triangles at u),
 * indexed by the vertex ids of the uploaded CSR.  Runs on the k = 3 bit-matrix kernels (one atomic per pivot member); pivots with
 * d+ > 8192 — none on RMAT up to scale 27 (max d+ = 3855) — run on the generic list recursion (one atomic per triangle, those pivots only). */
int gmsx_tc_vertex_count2(const gmsx_graph *g, int64_t *counts /* n, host */, gmsx_stats *stats);

/* ---- generic batched Set::intersect_count (sorted_set.h:176-182 / roaring_set.h:144-152) over graph rows:
 * out[i] = |N(u[i]) ∩ N(v[i])| on the full rows.  u, v, out are host arrays. */
int gmsx_intersect_count_batch(const gmsx_graph *g, int64_t n_pairs, const int32_t *u, const int32_t *v,
                               uint32_t *out, gmsx_stats *stats);
/* Set::intersect / Set::difference (sorted_set.h:160-197 -> sorted_set_operations.h:16-42, 73-99) MATERIALISED for a batch of vertex pairs —
 * result i = N(u[i]) ∩ N(v[i]) or N(u[i]) \ N(v[i]), ascending vertex ids of the uploaded CSR, CSR-shaped: out_offsets[n_pairs + 1] (host, always
 * filled) and out_ids (host).  out_ids == NULL is the sizing call (count pass + scan only); with out_ids the result must fit out_capacity ids, else
 * GMSX_ERR_INVALID (out_offsets[n_pairs] says how many it needs).  Two passes of one wave per pair (count, scan, fill): the base of the listing
 * consumers (BK without BK_COUNT, tomita.h:75-84; k-clique-star output, k_clique_star_list/parallel/output.h:14-68). */
enum { GMSX_SETOP_INTERSECT = 0, GMSX_SETOP_DIFFERENCE = 1 };
int gmsx_set_op_batch(const gmsx_graph *g, int op, int64_t n_pairs, const int32_t *u, const int32_t *v, int64_t *out_offsets /* n_pairs + 1 */,
                      int32_t *out_ids /* may be NULL */, int64_t out_capacity, gmsx_stats *stats);

/* ---- vertex similarity over graph rows: GMS::VertexSim::vertex_similarity<Metric> (gms/algorithms/set_based/vertex_similarity/
 * vertex_similarity.h:30-222), the scores behind the reference's link-prediction driver.  out[i] = metric(N(u[i]), N(v[i])) in
 * double precision, formulas as the reference writes them (its Jaccard divides by |A|+|B|+|A∩B|, :34-35).  The count-based
 * metrics are bit-identical to the reference; Adamic-Adar / resource-allocation sum their terms in a different order and use
 * the device log(): |rel. error| <= 1e-12. */
enum {
    GMSX_SIM_JACCARD = 0, GMSX_SIM_OVERLAP = 1, GMSX_SIM_ADAMIC_ADAR = 2, GMSX_SIM_RESOURCE = 3,
    GMSX_SIM_COMMON_NEIGHBORS = 4, GMSX_SIM_TOTAL_NEIGHBORS = 5, GMSX_SIM_PREF_ATTACHMENT = 6
};
int gmsx_vertex_similarity_batch(const gmsx_graph *g, int metric, int64_t n_pairs, const int32_t *u, const int32_t *v,
                                 double *out, gmsx_stats *stats);

/* ---- k-clique counting: CliqueCount (k_clique_count/k_clique_count_set_based.h:19-31).
 * *ordered_count = the reference's return value k!·C_k (mod 2^64, like size_t); *cliques = C_k (may be NULL).
 * k = 2 … 64.  The fast path — one bit-matrix per pivot — holds oriented out-degrees d+ <= 8192 for k <= 4, <= 4096 for
 * 5 <= k <= 10 (RMAT scale 26: max d+ = 3004); wider pivots and k > 10 run on a generic list recursion on the device (an order of
 * magnitude slower per pivot, same result), so no request fails for its size.  k > 64 → GMSX_ERR_UNSUPPORTED. */
int gmsx_kclique_count(const gmsx_graph *g, int k, uint64_t *ordered_count, uint64_t *cliques, gmsx_stats *stats);
int gmsx_kclique_partial(const gmsx_graph *g, int k, int part, int nparts, uint64_t *cliques_partial, gmsx_stats *stats);

/* ---- k-clique-star, COUNT mode: KCliqueStar::Par::CliqueStar<SGraph, OutputMode::Count>
 * (set_based/k_clique_star_list/parallel/recursive.h:19-35 over sequential/recursive.h:31-71).  The reference lists, for every k-clique
 * (reached once, members ascending), the clique and its STAR — the common neighbours of all its members outside it.
 * *stars = the number of (clique, star) pairs = C_k — what the reference prints as "total k-cliques" and what `output.size()` is;
 * *star_members = the total cardinality of the stars = (k+1)·C_{k+1}: every (k+1)-clique puts each of its members into the star of the
 * k-clique of the others (may be NULL: the (k+1)-clique pass is then skipped).  Both from the k-clique kernels above; the listing itself
 * is gmsx_kclique_star_list below.  k = 1 … 63. */
int gmsx_kclique_star_count(const gmsx_graph *g, int k, uint64_t *stars, uint64_t *star_members, gmsx_stats *stats);

/* ---- k-clique-star LISTING: KCliqueStar::Par::CliqueStarList (k_clique_star_list/parallel/recursive.h:37-43 over sequential/recursive.h:31-71).
 * One (clique, star) pair per k-clique of the graph: the k members, and the star — every vertex outside the clique that is adjacent to all
 * k members in the full undirected graph.  k = 1 gives (v, N(v)) for every vertex, isolated ones included (an empty star).  The sum of the
 * star sizes is (k+1)·C_(k+1), what gmsx_kclique_star_count reports.  With GMSX_KCSTAR_CLIQUES_ONLY the stars are not computed: k-clique
 * listing (k = 3: triangle listing); the star pointers must then be NULL (else GMSX_ERR_INVALID) and info->star_members = max_star = 0.
 * k = 1 … 63; k < 1 → GMSX_ERR_INVALID, k > 63 → GMSX_ERR_UNSUPPORTED.
 * All ids are vertex ids of the uploaded CSR.  Row i of `cliques` (k ids) is clique i, strictly ascending; star i is
 * star_members[star_offsets[i] .. star_offsets[i+1]), strictly ascending, star_offsets[0] = 0.
 * Two calls:
 *   sizing  all three arrays NULL: only *info is filled (info is required on every call);
 *   fill    cliques_capacity >= info.cliques (in cliques) and star_capacity >= info.star_members (in ids; star_members may be NULL if that
 *           is 0), else GMSX_ERR_INVALID with *info holding the required sizes and no buffer written.
 * A fill call that follows the sizing call of the same handle, k, flags and shard re-uses its first pass (one search instead of two).
 * Order: the PIVOT of a clique is its member that comes last in the device's degree order (decreasing (degree, id)).  The pairs of one
 * pivot are contiguous, pivots in that degree order; inside a pivot by the member chosen first — the pivot's neighbours that come before it
 * in the degree order, in ascending vertex id — then depth-first, every further member chosen in ascending vertex id among the common
 * neighbours that come before the member chosen last.  The same graph, upload flags, k, flags, part and nparts give byte-identical
 * arrays, in every process.
 * Shards: a shard is a set of whole pivots.  Pivot v belongs to part shard_of(p) where p is v's position in that degree order and
 * shard_of(p) = p mod nparts on even stripes p / nparts, nparts - 1 - (p mod nparts) on odd ones (the rule of gmsx_bk_list).  The parts of
 * one nparts are disjoint and their union is the whole list; (0, 1) is the whole graph; other (part, nparts) → GMSX_ERR_INVALID.
 * Width: every level set of a search is a list in a global slab, so no request is refused for the width of a neighbourhood.  The output of
 * a call is assembled on the device first: one that does not fit there returns GMSX_ERR_DEVICE_MEM and the caller uses more shards.  Test
 * hook: option KCSTAR_SLAB_MB.  Errors inside a pass (a slab or output bound, a fill that disagrees with its sizing pass) are reported as
 * GMSX_ERR_KERNEL; nothing is written out of bounds.
 * gmsx_stats: kernel_ms (the search passes), setup_ms (building the task list on the host), launches, units = tasks (pivot, first member). */
enum { GMSX_KCSTAR_DEFAULT = 0, GMSX_KCSTAR_CLIQUES_ONLY = 1 };
typedef struct {
    int64_t cliques;       /* k-cliques of this shard = (clique, star) pairs */
    int64_t star_members;  /* sum of the star sizes; 0 with CLIQUES_ONLY */
    int32_t k;
    int32_t max_star;      /* largest star listed; 0 with CLIQUES_ONLY */
} gmsx_kclique_star_list_info;
int gmsx_kclique_star_list(const gmsx_graph *g, int k, uint32_t flags, int part, int nparts,
                           int32_t *cliques /* k * info->cliques ids, row i = clique i, host, or NULL */,
                           int64_t *star_offsets /* info->cliques + 1, host, or NULL */, int32_t *star_members /* info->star_members, host, or NULL */,
                           int64_t cliques_capacity /* in cliques */, int64_t star_capacity /* in ids */,
                           gmsx_kclique_star_list_info *info /* required */, gmsx_stats *stats);

/* ---- Bron–Kerbosch maximal-clique count: BkEppsteinPar::mceBench with -DBK_COUNT
 * (maximal_clique_enum/parallel/eppsteinPAR.h:18-53 over sequential/tomita.h:12-86).
 * rank: n entries in rank format (host), or NULL.  The number of maximal cliques does not depend on the order the start
 * vertices split their neighbourhoods by (eppsteinPAR.h:39-45), so the device always splits by its own degree rank (the
 * order its containers are built for); a non-NULL `rank` is only VALIDATED — it must be a permutation of 0..n-1, else
 * GMSX_ERR_INVALID — the way the reference's drivers hand a rank vector from the preprocessing step to mceBench
 * (maximal_clique_enum_bron_kerbosch.cc:36-56).  gmsx_adg_rank() below is that preprocessing step on the device.
 * Width: start vertices with up to 16384 candidates (d+ in the device's degree rank; RMAT scale 27: max d+ = 3855) run on the
 * register-resident search kernels (1, 2, 4 or 8 words per lane, re-split across waves when a search outgrows its node budget);
 * wider ones run on a memory-resident search — one wave per start vertex, every level's sets in a global slab, an order of
 * magnitude slower per node, same count — so no graph is refused for the width of a neighbourhood. */
int gmsx_bk_count(const gmsx_graph *g, const int32_t *rank, uint64_t *maximal_cliques, gmsx_stats *stats);
int gmsx_bk_partial(const gmsx_graph *g, const int32_t *rank, int part, int nparts, uint64_t *partial, gmsx_stats *stats);

/* ---- Bron–Kerbosch maximal-clique LISTING: BkEppsteinPar::mceBench without -DBK_COUNT (eppsteinPAR.h:18-53, tomita.h:79-84 fill `sol`).
 * The cliques listed are exactly the reference's: every maximal clique of the graph once, an isolated vertex v as {v}.  Members are the
 * vertex ids of the uploaded CSR, strictly ascending inside each clique; clique i is members[offsets[i] .. offsets[i+1]), offsets[0] = 0.
 * rank: validated exactly as by gmsx_bk_count (NULL, or a permutation of 0..n-1, else GMSX_ERR_INVALID); the set does not depend on it.
 * Two calls:
 *   sizing  offsets == NULL and members == NULL: only *info is filled (info is required on every call);
 *   fill    offsets_capacity >= info.cliques + 1 and members_capacity >= info.members (members may be NULL if that is 0), else
 *           GMSX_ERR_INVALID with *info holding the required sizes and neither buffer written.
 * A fill call that follows the sizing call of the same handle and shard re-uses its first pass (one search instead of two).
 * Order: the cliques of one start vertex are contiguous, start vertices in the device's degree order (decreasing (degree, id)); inside one
 * start vertex the depth-first order of its search.  The same graph, upload flags, part and nparts give byte-identical arrays, in every
 * process.
 * Shards: start vertex v belongs to part shard_of(p) where p is v's position in that degree order and shard_of(p) = p mod nparts on even
 * stripes p / nparts, nparts - 1 - (p mod nparts) on odd ones; a clique is listed by its member of the lowest position.  The shards of one
 * nparts are disjoint and their union is the whole list; (0, 1) is the whole graph.  A shard can be listed (and freed) at a time, so an
 * output larger than host memory can be streamed.
 * Width: every start vertex runs the same memory-resident search (a global slab of Cadj | XT | levels per start vertex), so no graph that
 * gmsx_bk_count accepts is refused for the width of a neighbourhood.  Test hook: option BK_LIST_ARENA_MB (budget of the slabs of one
 * launch; smaller = more launches).  Errors inside a pass (a slab or output bound, a fill that disagrees with its sizing pass) are
 * reported as GMSX_ERR_KERNEL; nothing is written out of bounds. */
typedef struct {
    int64_t cliques;        /* maximal cliques of this call's shard */
    int64_t members;        /* sum of their sizes = entries `members` needs */
    int32_t max_size;       /* largest clique listed (0 if none) */
    int64_t size_hist[65];  /* [s] = cliques with s members for s < 64, [64] = 64 or more; [0] = 0 */
} gmsx_bk_list_info;
int gmsx_bk_list(const gmsx_graph *g, const int32_t *rank, int part, int nparts, int64_t *offsets /* info->cliques + 1 entries, host, or NULL */,
                 int32_t *members /* info->members entries, host, or NULL */, int64_t offsets_capacity, int64_t members_capacity,
                 gmsx_bk_list_info *info /* required */, gmsx_stats *stats);

/* ---- vertex orderings that consume the path's operators ----
 * PpParallel::getDegeneracyOrderingApproxSGraph<boundary_function::averageDegree> (preprocessing/parallel/
 * degeneracy_approx_set.h:14-86, boundary_function.h:14-23): peel in rounds — every remaining vertex whose remaining degree is
 * <= (unsigned)((1+epsilon) * average remaining degree) leaves in this round; the degrees of the others drop by
 * |N(v) ∩ X| (the intersect_count of :77).  out[n] (host): rank_format != 0 → out[v] = position of v (what BK consumes,
 * eppsteinPAR.h:41), else out[i] = i-th vertex.  *rounds (may be NULL) = number of peeling rounds.
 * Ties: inside a round the vertices are ordered by (remaining degree, vertex id).  The reference leaves ties to
 * __gnu_parallel::partition / sort (:41-59), i.e. to the thread count; every order it can produce has the same rounds and the
 * same remaining-degree sequence as this one. */
int gmsx_adg_rank(const gmsx_graph *g, double epsilon, int rank_format, int32_t *out, int32_t *rounds, gmsx_stats *stats);
/* PpParallel::triangleCountOrdering (preprocessing/parallel/triangle_count.h:11-30): ordering[i] = i-th vertex by increasing
 * per-vertex count (the counts of gmsx_tc_vertex_count2); ties by vertex id (the reference's std::sort leaves them open).
 * (As shipped, the reference's default CountFn vertex_count2_once adds into an uninitialised pvector, triangle_count.h:19 +
 * parallel/vertex.h:42-46, so its own output depends on heap contents; this is the ordering by the well-defined counts, which
 * the reference produces with CountFn = Par::vertex_count2 — that instantiation is what the goldens were generated with.) */
int gmsx_tc_ordering(const gmsx_graph *g, int32_t *ordering /* n, host */, gmsx_stats *stats);

/* ---- exact k-core decomposition and an exact degeneracy order: the device counterpart of PpSequential::getDegeneracyOrderingMatula
 * (preprocessing/sequential/degeneracy_matula.h:13-66; PpParallel::getDegeneracyOrderingMatula, parallel/degeneracy_matula.h, is the same serial
 * loop behind a parallel degree pass) — "BK-GMS-DGR" of the Bron–Kerbosch driver (maximal_clique_enum_bron_kerbosch.cc:50-56).
 * The peel: k = 0, every vertex remaining.  While vertices remain, k rises to the smallest remaining degree; then rounds repeat until none
 * applies: in one round every remaining vertex whose remaining degree is <= k leaves at once — its core number is k, its round the running
 * round index — and the remaining degrees of its still-remaining neighbours drop.  Isolated vertices leave in round 0 with core number 0.
 * core[v] (n, host, or NULL) is unique for the graph: the running maximum of the removal degrees along the reference's Matula order, bit for bit;
 * info->degeneracy = its maximum = CoreNumberEvaluator::getCoreNumberOfOrder of that order (core_number_evaluator.h:115-139).
 * ordering (n, host, or NULL): the vertices by ascending (round, vertex id); rank_format as in gmsx_adg_rank (!= 0: ordering[v] = position of v,
 * else ordering[i] = i-th vertex).  Every vertex has at most core[v] <= degeneracy neighbours after it, so this IS an exact degeneracy order: it
 * passes DegeneracyOrderingVerifier::degegeneracyOrderingVerifier (preprocessing/verifiers/degeneracy_verifier.h:70-86) and, handed to
 * Bron–Kerbosch as the rank, bounds every candidate set by the degeneracy.
 * Ties: it is NOT Matula's own sequence.  That one takes, step by step, the minimum of (remaining degree, id) among the remaining vertices
 * (:39-45, the first element of the lowest non-empty bucket) and is serial by construction; all exact degeneracy orders share the core
 * numbers and the bound, and this one is the one a level-synchronous peel defines.  The same graph gives byte-identical core, ordering and
 * info in every process and on every run (the arrival order of the atomics reaches no output).
 * core and ordering may both be NULL: only *info is filled.  n = 0: GMSX_OK, *info zeroed.  NULL g or info: GMSX_ERR_INVALID.  A frontier that
 * would overflow its buffer or a final count != n is reported as GMSX_ERR_KERNEL; nothing is written out of bounds.  Test hook: option
 * CORE_WG_FRONTIER.  gmsx_stats: kernel_ms, launches, units = n, probes = rounds. */
typedef struct {
    int32_t degeneracy;   /* largest core number = the graph's degeneracy; 0 for an edgeless graph */
    int32_t levels;       /* distinct core numbers that occur */
    int32_t rounds;       /* peel rounds (definition above) */
    int32_t reserved;
    int64_t top_core;     /* vertices whose core number equals degeneracy */
} gmsx_core_info;
int gmsx_core_decomposition(const gmsx_graph *g, int32_t *core /* n, host, or NULL */, int32_t *ordering /* n, host, or NULL */, int rank_format,
                            gmsx_core_info *info /* required */, gmsx_stats *stats);
/* PpParallel::getDegreeOrdering (preprocessing/parallel/degree.h:15-61) — "BK-GMS-DEG" (maximal_clique_enum_bron_kerbosch.cc:43-49): the
 * vertices by ASCENDING (degree, vertex id).  compare_degree (:16-22) is a strict total order, so the result is the reference's bit for bit in
 * both formats (rank_format as in gmsx_adg_rank).  Not the device's internal degree order (that one is decreasing). */
int gmsx_degree_rank(const gmsx_graph *g, int rank_format, int32_t *out /* n, host */, gmsx_stats *stats);
/* CoreNumberEvaluator (preprocessing/util/core_number_evaluator.h): how good an order is as a degeneracy order.
 * ordering: n entries (host), rank_format as in gmsx_adg_rank; it must be a permutation of 0..n-1 (checked on the device), else
 * GMSX_ERR_INVALID and nothing is written.  core_number: the degeneracy to grade against; < 0 = computed here by the peel of
 * gmsx_core_decomposition.  later (n, host, or NULL): per vertex the number of its neighbours that come after it.
 * With core_number = 0 (an edgeless graph) the three doubles are 0.0 — the reference divides by zero there (:108-110).  n = 0: GMSX_OK, the
 * integers 0 (core_number as passed, 0 if < 0), the doubles 0.0. */
typedef struct {
    int32_t max_later;            /* CoreNumberEvaluator::getCoreNumberOfOrder (:115-139): max over v of |{w in N(v): w after v}| */
    int32_t core_number;          /* the degeneracy the order was graded against */
    int32_t core_number_of_order; /* evaluateCoreNrAccuracy (:73-112): max(core_number, max_later) */
    int32_t reserved;
    int64_t faulty;               /* vertices with more than core_number neighbours after them (biggerThanCore) */
    int64_t excess;               /* sum over those of (later - core_number) (difAcc, in 64 bits; the reference's unsigned int wraps above 2^32) */
    double relative_error, fault_rate, relative_mean_difference; /* the reference's three expressions (:108-110), evaluated on the host from the integers above, operand order as written there */
} gmsx_order_quality_info;
int gmsx_order_quality(const gmsx_graph *g, const int32_t *ordering /* n, host */, int rank_format,
                       int32_t core_number /* < 0: computed here by the peel of gmsx_core_decomposition */,
                       int32_t *later /* n, host, or NULL: per-vertex count of neighbours after v */,
                       gmsx_order_quality_info *info /* required */, gmsx_stats *stats);

/* ---- graph colouring: GMS::Coloring::JonesV3::graph_coloring_jones (non_set_based/coloring/coloring_jones_v3.h:38-68), Jones–Plassmann under a
 * caller-given priority — what benchmarkGraphColoringWithReordering times (coloring.cc:82-129, :149).  u is a PREDECESSOR of v iff u is a neighbour
 * of v and order[u] > order[v] (:52); a vertex takes the smallest colour >= 1 that none of its predecessors holds (:12-21).  The result is a
 * function of (graph, order): the greedy colouring of the vertices taken by DESCENDING order[], the reference's array element for element at
 * every thread count.
 * ordering (n, host, or NULL): rank_format as in gmsx_adg_rank (!= 0: ordering[v] = position of v, else ordering[i] = i-th vertex).  The vertex of
 * the HIGHEST position is coloured first.  That is the convention of the rank producers here: gmsx_degree_rank gives largest-first (LF),
 * gmsx_core_decomposition's order smallest-last (SL: at most core[v] predecessors per vertex, so at most degeneracy + 1 colours), gmsx_adg_rank the
 * approximate SL.  NULL = order[v] = v, PpSequential::getSimpleIdOrdering, what coloring.cc:25-30 hands to JonesV3; order[v] = n-1-v gives
 * graph_coloring_naive_sequential (coloring_sequential.h:17-42), first-fit in id order.  ordering must be a permutation of 0..n-1 (checked on
 * the device), else GMSX_ERR_INVALID and nothing is written: the reference mis-colours on ties.
 * coloring (n, host, or NULL): coloring[v] in 1..info->colors.  round_of (n, host, or NULL): the Jones–Plassmann round of v — 0 without
 * predecessors, else 1 + the maximum over its predecessors (its depth in the priority DAG).
 * All outputs are a fact about (graph, permutation): byte-identical in every process and on every run (the arrival order of the atomics reaches
 * no output).  n = 0: GMSX_OK, *info zeroed.  NULL g or info: GMSX_ERR_INVALID.  A frontier that would overflow its buffer or a final coloured
 * count != n is reported as GMSX_ERR_KERNEL; nothing is written out of bounds and the caller's arrays are written only after success.
 * Width: the forbidden colours of a vertex are a bitmap in LDS for rows of up to 1024 entries and in a global slab beyond, so no graph is
 * refused for a wide neighbourhood.  A colouring is global: the call is single-GPU only, there are no shards.
 * Test hook: option COLOR_WG_FRONTIER.  gmsx_stats: kernel_ms, launches, units = n, probes = rounds. */
typedef struct {
    int32_t colors;      /* largest colour used = number of colours (greedy leaves no gap in 1..colors); 0 for n = 0 */
    int32_t rounds;      /* Jones–Plassmann rounds = vertices on the longest path of the priority DAG; 0 for n = 0 */
    int32_t max_pred;    /* most predecessors of any vertex (= gmsx_order_quality's max_later for this order); colors <= max_pred + 1 */
    int32_t reserved;
    int64_t first_round; /* vertices without a predecessor (the size of round 0) */
} gmsx_coloring_info;
int gmsx_coloring_jp(const gmsx_graph *g, const int32_t *ordering /* n, host, or NULL */, int rank_format,
                     int32_t *coloring /* n, host, or NULL */, int32_t *round_of /* n, host, or NULL */,
                     gmsx_coloring_info *info /* required */, gmsx_stats *stats);
/* The reference's verifiers (coloring_common.h) as integers over any colouring (n, host):
 *   GCVerifierMaxColor(g, c, m) (:102-122)   <=>  invalid == 0 && conflicts == 0 && max_color <= m
 *   GCVerifierDeltaPlusOne (:125-157)        <=>  the same with m = max_degree + 1
 * One difference: a NEGATIVE colour counts as invalid here and passes the range test of GCVerifierMaxColor (c == 0 || c > maxColor, :109); no
 * reference algorithm produces one.  n = 0: GMSX_OK, *out zeroed.  NULL g, out or (n > 0) coloring: GMSX_ERR_INVALID. */
typedef struct {
    int64_t conflicts;   /* undirected edges {u,v} with coloring[u] == coloring[v] */
    int64_t invalid;     /* vertices with coloring[v] < 1 */
    int32_t max_color, distinct;   /* distinct = the reference's uniqueColorsCount (coloring_common.h:205-209) */
    int32_t max_degree, reserved;
} gmsx_coloring_check;
int gmsx_coloring_verify(const gmsx_graph *g, const int32_t *coloring /* n, host */, gmsx_coloring_check *out /* required */, gmsx_stats *stats);

/* ---- per-edge triangle support and the exact k-truss decomposition: the edge counterpart of gmsx_tc_vertex_count2 and gmsx_core_decomposition.
 * No reference counterpart (the k-truss is the member of the k-core / k-clique / k-clique-star / k-truss family the reference lists and does not
 * build); both are one Set::intersect_count per edge, and the peel below is the k-core peel one level up.
 * SUPPORT.  support(e) of an undirected edge e = {u, v} is |N(u) ∩ N(v)| on the full rows: the number of triangles through e.
 * THE PEEL.  l = 0, every edge remaining.  While edges remain, l rises to the smallest remaining support; then rounds repeat until none
 * applies: in one round every remaining edge whose remaining support is <= l leaves at once — its trussness is l + 2, its round the running
 * round index.  A triangle is destroyed if all three of its edges were remaining at the start of the round and at least one of them leaves;
 * the remaining support of each of its edges that does not leave in this round drops by one — once per triangle, however many of its edges
 * leave.  truss(e) is therefore the largest k such that e lies in a subgraph whose every edge is in at least k - 2 triangles of that subgraph
 * ({e : truss(e) >= k} is the k-truss); every edge has truss >= 2.
 * Per-arc outputs (nnz, host) are parallel to the uploaded CSR's neigh: entry j belongs to arc j, and the two arcs of an edge carry the same
 * value.  support, truss, round_of, rounds and levels are facts about the graph: byte-identical in every process and on every run (the arrival
 * order of the atomics reaches no output).  The caller's arrays are written only after success.
 * n = 0 or no edge: GMSX_OK, *info zeroed (*triangles = 0).  NULL g, NULL info, or NULL support with nnz > 0: GMSX_ERR_INVALID, nothing written.
 * m >= 2^31: GMSX_ERR_UNSUPPORTED — edge ids are 32 bits (no test reaches this branch: such a graph does not fit a test).  A CSR that is not
 * symmetric and loop-free (possible only under GMSX_UPLOAD_TRUSTED), a frontier that would overflow its buffer or a final count != m is reported
 * as GMSX_ERR_KERNEL; nothing is written out of bounds.  Both calls are single-GPU only, there are no shards (a sharded upload gives the same bytes).
 * Test hook: option TRUSS_WG_FRONTIER.  gmsx_stats of gmsx_truss_decomposition: kernel_ms (the peel), setup_ms (edge numbering and support),
 * launches, units = m, probes = rounds; of gmsx_edge_support: kernel_ms (edge numbering and support), launches, units = m. */
typedef struct {
    int32_t max_truss;    /* largest trussness; 0 for a graph without edges, 2 for a triangle-free one */
    int32_t levels;       /* distinct trussness values that occur */
    int32_t rounds;       /* peel rounds (definition above) */
    int32_t max_support;
    int64_t top_edges;    /* undirected edges with truss == max_truss */
    int64_t triangles;    /* (sum of support over undirected edges) / 3 */
} gmsx_truss_info;
int gmsx_edge_support(const gmsx_graph *g, int32_t *support /* nnz, host */, uint64_t *triangles /* may be NULL */, gmsx_stats *stats);
int gmsx_truss_decomposition(const gmsx_graph *g, int32_t *truss /* nnz, host, or NULL */, int32_t *round_of /* nnz, host, or NULL */,
                             gmsx_truss_info *info /* required */, gmsx_stats *stats);

/* ---- link prediction: GMS::LinkPrediction::link_prediction_similarity<Metric> (set_based/link_prediction/link_prediction.h:42-101), the q
 * best-scoring NON-edges of the graph under one of the GMSX_SIM_* metrics, and the precision / recall step of the reference's bench_ranking
 * (link_prediction.cc:30-49).  The reference walks all pairs u < v in lexicographic order, skips edges and inserts each score into an ascending
 * array of q slots with a strict `>`; that is exactly this rule:
 *   candidates  the non-edges u < v whose score is not NaN (Overlap is 0/0 when an endpoint is isolated, vertex_similarity.h:64-66: never inserted)
 *   order       decreasing score, ties by ascending (u, v)
 *   result      the first min(q, candidates) of that order, returned in REVERSE: index 0 is the worst entry kept, the last index the best.
 * Scores are those of gmsx_vertex_similarity_batch, bit for bit (one device function computes both), including the reference's Jaccard
 * c/(|A|+|B|+c), which is 1.0 when both rows are empty.  u, v, scores (host, `capacity` entries each) receive info->found = min(q, candidates)
 * entries; one call does everything, there is no sizing call.  The reference leaves q - found leading entries (-1.0, edge (0,0)) when fewer than
 * q candidates exist and returns exactly one such entry when none does: the C call returns the real entries only, gmsx::link_prediction
 * (gmsx_set_graph.hpp) reproduces the padding.
 * Classes: for Jaccard, Overlap, Adamic-Adar, Resource and CommonNeighbors a non-edge is ONE (Jaccard only: both endpoints isolated, 1.0), POS (at
 * least one common neighbour, score > 0; every such Jaccard score is <= 1/3) or ZERO (no common neighbour, exactly 0.0; Overlap: both endpoints
 * non-isolated); the order is ONE, POS, ZERO, and inside ONE and ZERO purely lexicographic.  Only POS pairs — found by two-hop marking per
 * source vertex — are scored and sorted; ZERO is generated in order, chunk by chunk, until q is reached.  TotalNeighbors and PrefAttachment rank
 * every non-edge (one class, ALL).
 * Cost: the ALL class, and a ZERO fill that cannot stop early (q above the POS pairs plus most ZERO pairs), cost O(n^2) scores / pairs, as the
 * reference does; the ALL class returns GMSX_ERR_UNSUPPORTED for n > 131072.  q > 2^27 returns GMSX_ERR_UNSUPPORTED.
 * Shards: a shard owns the sources u with u mod nparts == part; (0, 1) is the whole graph.  Merging the shards' outputs under the rule and
 * truncating to q gives the whole graph's output byte for byte (capi.merge_link_predictions, gmsx::merge_link_predictions).
 * The same graph, metric, q and shard give byte-identical arrays in every process: the arrival order of atomics reaches no output (the
 * two-hop bitmaps are set by idempotent ORs, candidates leave them in ascending v, and equal scores are ordered by one STABLE sort).
 * Errors: q < 1, an unknown metric, a NULL g, info or output array, capacity < min(q, 2^62), part / nparts outside 0 <= part < nparts →
 * GMSX_ERR_INVALID, nothing written.  A bounds violation or a fill that disagrees with its count pass → GMSX_ERR_KERNEL; nothing is written
 * out of bounds and the caller's arrays are written only after the device flag word was read as zero.  n = 0 or 1: GMSX_OK, found = 0.
 * Test hooks: options LP_LDS_MAXN, LP_SLAB_MB.  gmsx_stats: kernel_ms (the device span of the call), launches, units = scored. */
typedef struct {
    int64_t found;        /* entries written: min(q, candidates) */
    int64_t scored;       /* pairs whose score was computed */
    int64_t positive;     /* POS pairs of this shard (five common-neighbour metrics); -1 where the ALL class ran */
    int32_t chunks;       /* launches-of-sources the call was cut into: the POS / ALL and ZERO chunks that were filled (0 when ONE alone filled q) */
    int32_t classes;      /* bit 0 ONE, 1 POS, 2 ZERO, 3 ALL: which classes contributed to the output */
} gmsx_link_prediction_info;
int gmsx_link_prediction(const gmsx_graph *g, int metric /* GMSX_SIM_* */, int64_t q, int part, int nparts,
                         int32_t *u /* capacity */, int32_t *v /* capacity */, double *scores /* capacity */,
                         int64_t capacity, gmsx_link_prediction_info *info /* required */, gmsx_stats *stats);
/* score_link_prediction_precision (evaluation.h:99-124): g_test's undirected edges against a predicted list u[i], v[i] (host, n_pred entries).
 * (u, v) and (v, u) are the same edge; duplicates in the list count once, as EdgeSet.contains over g_test's edges implies.  *true_positives =
 * the edges of g_test that occur in the list, *true_count = the edges of g_test, *precision = tp / n_pred, *recall = tp / true_count: plain
 * double divisions on the host; where a denominator is 0 the reference divides by zero — 0.0 here.  Every output pointer may be NULL.
 * A pair with u == v or an id outside [0, n) → GMSX_ERR_INVALID.  n_pred = 0 is allowed. */
int gmsx_link_prediction_precision(const gmsx_graph *g_test, int64_t n_pred, const int32_t *u, const int32_t *v,
                                   int64_t *true_positives, int64_t *true_count, double *precision, double *recall,
                                   gmsx_stats *stats);

/* ---- subgraph matching: GMS::SubGraphIso::VF2 (non_set_based/subgraphiso/vf2/sequential/vf2.hpp:53-81 with the candidate rule of
 * vf2/util/candidateGeneration.hpp:12-56 and the feasibility rules of vf2/util/feasibilityRules.hpp:48-92), and the enumeration the reference's
 * drivers stop short of: EVERY embedding of a small connected pattern P into the uploaded graph G, as rows of one array.
 * Pattern: a symmetric CSR over k vertices — int64 p_offsets[k + 1], int32 p_neigh[p_offsets[k]], rows strictly ascending, loop-free, the arc set
 * equal to its transpose — validated on the host on every call: a violation (an id outside [0, k) included) → GMSX_ERR_NOT_CANONICAL.
 * 1 <= k <= 32: k < 1 or a NULL array → GMSX_ERR_INVALID, k > 32 → GMSX_ERR_UNSUPPORTED.  The pattern must be connected; a disconnected one →
 * GMSX_ERR_UNSUPPORTED (its candidate sets are not subsets of a row).  No vertex or edge labels.
 * Embedding: an injective f : V(P) → V(G).  INDUCED (the default; what VF2 decides, feasibilityRules.hpp:48-92): {a, b} ∈ E(P) <=> {f(a), f(b)} ∈
 * E(G).  GMSX_SGM_MONO: only => is required — the non-induced mode of the reference's verifier (util/subgraphiso_verification.hpp:11-78,
 * isInducedIsomorphism = false).  Every embedding is listed, so one subgraph copy appears |Aut(P)| times; there is no symmetry breaking.
 * Matching order pi: pi_0 = 0, pi_(i+1) = the smallest pattern vertex adjacent to {pi_0 .. pi_i}; every pi_i, i >= 1, has an earlier neighbour.
 * It is the order the reference's candidate rule walks a connected pattern in; info->order and gmsx_subgraph_order (host only, no device needed;
 * the same status codes as above) return it.
 * Output: row i of `maps` (k ids) is embedding i, column p holds f(p) — indexed by pattern vertex id, not by position in pi; all ids are vertex
 * ids of the uploaded CSR.  Rows are in ascending lexicographic order of (f(pi_0), f(pi_1), .., f(pi_(k-1))).  In INDUCED mode row 0 is the
 * reference's sequential VF2 result (Result::isomorphism), element for element: its depth-first search takes the pattern vertices in the order
 * pi and the target vertices ascending and stops at the first embedding it meets (vf2.hpp:53-81).  (The reference's parallel driver returns
 * whichever embedding its tasks meet first; only its existence answer is a fact about the input.)  The same graph, pattern, flags and shard
 * give byte-identical arrays in every process.
 * Two calls, as gmsx_kclique_star_list:
 *   sizing  maps == NULL: only *info is filled (info is required on every call); it always searches;
 *   fill    capacity >= info.embeddings (in embeddings), else GMSX_ERR_INVALID with *info holding the need and nothing written.
 * A fill call that follows the sizing call of the same handle, pattern (the arrays are compared in full), flags and shard re-uses its first
 * pass.  The output is assembled on the device first: one that does not fit there returns GMSX_ERR_DEVICE_MEM and the caller uses more shards.
 * GMSX_SGM_FIRST (combinable with MONO): the reference driver's question — is there one, and which.  One call, no sizing: info.embeddings is 0
 * or 1; with maps != NULL capacity >= 1 is required and the one row written is row 0 of the full list; maps == NULL answers existence only.  The
 * search stops early: a task that meets its first embedding records its task index by an atomic minimum and ends, every task quits once a lower
 * task has recorded one, and the host launches ascending ranges of tasks and stops after the first launch that found one.  Timing decides only
 * how much abandoned work is done, never the result.
 * Shards: an embedding belongs to part shard_of(f(pi_0)) — the rule of gmsx_kclique_star_list applied to the vertex id of the first image.  The
 * parts of one nparts are disjoint and their row-wise merge in the list order is the whole list; (0, 1) is the whole graph; other (part, nparts)
 * → GMSX_ERR_INVALID.
 * Width: the candidates of a level are computed 64 ids at a time straight from one row of the CSR and never stored, so no request is refused for
 * the width of a neighbourhood.  Test hook: option SGM_LAUNCH_TASKS (tasks per launch; the defaults, 2^24 and 2^16 with FIRST, are first guesses,
 * not tuned values).
 * Errors: unknown flag bits, a NULL g or info, a negative capacity → GMSX_ERR_INVALID.  A fill that disagrees with its count pass, or an output
 * bound → GMSX_ERR_KERNEL; nothing is written out of bounds and the caller's array is written only after the device flag word was read as zero.
 * n = 0 or k > n: GMSX_OK with 0 embeddings.
 * gmsx_stats: kernel_ms (the search passes), setup_ms (building the task list on the host), launches, units = tasks — the arcs (f(pi_0), f(pi_1))
 * that pass the degree filters d(f(p)) >= deg_P(p); k = 1: the vertices. */
enum { GMSX_SGM_INDUCED = 0, GMSX_SGM_MONO = 1, GMSX_SGM_FIRST = 2 };
typedef struct {
    int64_t embeddings;   /* of this call's shard; with FIRST: 0 or 1 */
    int64_t tasks;
    int32_t k, reserved;
    int32_t order[32];    /* the matching order pi (pattern vertex ids), k entries, the rest -1 */
} gmsx_subgraph_info;
int gmsx_subgraph_order(int32_t k, const int64_t *p_offsets, const int32_t *p_neigh, int32_t *order /* k */);
int gmsx_subgraph_match(const gmsx_graph *g, int32_t k, const int64_t *p_offsets, const int32_t *p_neigh, uint32_t flags, int part, int nparts,
                        int32_t *maps /* k * capacity ids, row i = embedding i, host, or NULL */, int64_t capacity /* in embeddings */,
                        gmsx_subgraph_info *info /* required */, gmsx_stats *stats);

/* ---- connected components and Jarvis–Patrick clustering: one device union-find over the vertices of the uploaded CSR.
 * gmsx_connected_components is ShiloachVishkin (gms/representations/graphs/log_graph/cc.cc:40-72): label[v] is the smallest vertex id of v's
 * component, which is what the reference's hooking of larger labels under smaller ones converges to; so label[v] <= v and
 * label[label[v]] == label[v].  gmsx_jarvis_patrick has no reference counterpart (like the k-truss it is the member of the family the suite
 * describes and does not build): keep an edge {u, v} iff metric(N(u), N(v)) >= threshold on the full rows; the clusters are the connected
 * components of what is kept.
 * arc_keep AS AN INPUT (gmsx_connected_components; NULL = every edge): nnz bytes parallel to the uploaded CSR's neigh, like the per-arc arrays of
 * gmsx_truss_decomposition.  An edge is kept if the byte of at least one of its two arcs is non-zero, so a symmetric mask (truss >= k) and a
 * one-sided one both mean what they look like.  info->kept_edges counts each kept edge once (an arc u -> v with u > v counts only if the byte of
 * v -> u is zero).
 * arc_keep AS AN OUTPUT (gmsx_jarvis_patrick; may be NULL): symmetric, 0 or 1.  Fed back into gmsx_connected_components it gives the same labels
 * and info, byte for byte.
 * Scores are those of gmsx_vertex_similarity_batch, bit for bit (one device function computes both); a NaN score (Overlap of an isolated
 * endpoint cannot occur on an edge, but the rule stands) is never kept.  All seven GMSX_SIM_* metrics are accepted; GMSX_SIM_COMMON_NEIGHBORS
 * with an integer threshold k is the classical "share at least k neighbours".  Note that the reference's Jaccard, c / (|A| + |B| + c), never
 * exceeds 1/3.
 * label, every field of info except passes, and the output mask are facts about the graph: byte-identical in every process and on every run (the
 * arrival order of the atomics reaches no output).  The caller's arrays are written only after the device flag word was read as zero.
 * n = 0: GMSX_OK, *info zeroed.  A graph without edges or a mask of zeros: n singletons.  NULL g or info, an unknown metric or a NaN threshold:
 * GMSX_ERR_INVALID, nothing written.  Every walk and retry loop of the kernels is capped (n + 64 steps); a cap that is exceeded, a list that
 * would overflow or an arc without its twin (possible only under GMSX_UPLOAD_TRUSTED) is reported as GMSX_ERR_KERNEL, and nothing is written
 * out of bounds.  Single GPU, no shards — a component is global; a sharded upload gives the same bytes.
 * Test hooks: options CC_SAMPLE, CC_WAVE_ROW, CC_WG_ROW (first guesses, not tuned).  gmsx_stats: kernel_ms (linking and flatten), setup_ms (the
 * mask upload and the info reduction), launches, units = arcs the linking kernels examined (Jarvis–Patrick: edges scored = m), alg_elements =
 * Σ(d_u + d_v) over the scored edges (Jarvis–Patrick only). */
typedef struct {
    int64_t components;     /* connected components, singletons included */
    int64_t singletons;     /* components of one vertex */
    int64_t largest;        /* vertices in the largest component */
    int64_t kept_edges;     /* undirected edges the components were taken over */
    int32_t largest_label;  /* its label; ties: the smallest label */
    int32_t passes;         /* flatten rounds of the final pointer jumping (diagnostic; may differ between runs) */
} gmsx_components_info;
int gmsx_connected_components(const gmsx_graph *g, const uint8_t *arc_keep /* nnz, host, or NULL = every edge */,
                              int32_t *label /* n, host, or NULL */, gmsx_components_info *info /* required */, gmsx_stats *stats);
int gmsx_jarvis_patrick(const gmsx_graph *g, int metric /* GMSX_SIM_* */, double threshold,
                        int32_t *label /* n, host, or NULL */, uint8_t *arc_keep /* nnz, host, or NULL: out */,
                        gmsx_components_info *info /* required */, gmsx_stats *stats);

/* ---- breadth-first search and betweenness centrality (gms/representations/graphs/log_graph/bfs.cc: DOBFS, bc.cc: Brandes).
 * gmsx_bfs: depth[v] = distance from source (-1: unreachable); parent[v] = the SMALLEST-id neighbour of v at depth[v] - 1, parent[source] =
 * source, -1 for an unreachable vertex.  That is what the reference's bottom-up step writes (the first frontier entry of an ascending row), it
 * passes BFSVerifier (bfs.cc:212-258), and unlike the reference's top-down parents it is a fact about (graph, source): depth, parent and every
 * info field except bottom_up_levels are byte-identical in every run and process, under every BFS_* option, GMSX_UPLOAD_TRUSTED,
 * GMSX_UPLOAD_HUB_LIMIT and a sharded upload.  bottom_up_levels is a fact about (graph, source, options).  The levels are taken top-down (the
 * frontier-rounds engine) or bottom-up (every unvisited vertex scans its own row for a frontier bit) by the reference's rule, bfs.cc:142-188.
 * source outside [0, n) (hence any source when n = 0), NULL g or info: GMSX_ERR_INVALID, nothing written.  An append past its bound, a level count
 * above n, or `reached` disagreeing with the level sums: GMSX_ERR_KERNEL.  The caller's arrays are written only after the flag words were read as
 * zero.  Single GPU, no shards.  gmsx_stats: kernel_ms, setup_ms, launches, units = reached_arcs, probes = levels.
 * gmsx_betweenness: scores[u] = Σ_s delta_s(u) over the given sources, one after the other (a source listed twice counts twice, as bc.cc -r s -i 2),
 * delta_s(u) = Σ_{v in N(u), depth(v) = depth(u) + 1} sigma(u) / sigma(v) * (1 + delta_s(v)) — bc.cc:131-132, its operand order — with sigma the
 * number of shortest paths from s, in DOUBLE (the reference's 32-bit counts wrap; a 40 x 40 grid passes 2^64): exact while info->max_sigma < 2^53.
 * The default adds delta_s(s) = reached(s) - 1 to the source's own score as Brandes and BCVerifier do (bc.cc:124-138, 207-216);
 * GMSX_BC_EXCLUDE_SOURCE leaves it out (textbook Brandes; on an undirected graph with all n sources twice the unordered-pair value);
 * GMSX_BC_NORMALIZE_MAX divides by the largest score (bc.cc:144-151; an all-zero result stays zeros).  No floating-point atomic is used: a row's
 * sum is taken by fixed lanes over fixed strides and combined by a fixed tree, a score has one writer — scores is a fact about (graph, sources,
 * flags), byte-identical in every run and under every BFS_* option.  An id outside [0, n), unknown flag bits, NULL g / info, NULL scores with
 * n > 0 or NULL sources with n_sources > 0: GMSX_ERR_INVALID, nothing written.  n_sources = 0: zeros.  Single GPU.  gmsx_stats: kernel_ms,
 * setup_ms, launches, units = Σ reached_arcs, probes = Σ levels. */
typedef struct {
    int64_t reached;          /* vertices with depth >= 0, the source included */
    int64_t reached_arcs;     /* sum of their degrees */
    int64_t depth_sum;        /* sum of depth over the reached vertices (closeness = (reached-1)/depth_sum) */
    int64_t widest;           /* size of the largest level */
    int32_t levels;           /* non-empty levels = eccentricity of the source + 1 */
    int32_t widest_level;     /* its depth; ties: the smallest */
    int32_t bottom_up_levels; /* levels discovered by the bottom-up step: a fact about (graph, source, options) */
    int32_t reserved;
} gmsx_bfs_info;
int gmsx_bfs(const gmsx_graph *g, int32_t source, int32_t *depth /* n, host, or NULL */, int32_t *parent /* n, host, or NULL */,
             gmsx_bfs_info *info /* required */, gmsx_stats *stats);
enum { GMSX_BC_DEFAULT = 0, GMSX_BC_EXCLUDE_SOURCE = 1, GMSX_BC_NORMALIZE_MAX = 2 };
typedef struct {
    int64_t sources;       /* as passed */
    int64_t reached_total; /* sum over the sources of gmsx_bfs's reached */
    int32_t max_levels;    /* largest levels of any source */
    int32_t reserved;
    double  max_score;     /* before normalisation */
    double  max_sigma;     /* largest shortest-path count met; below 2^53 every count was exact */
} gmsx_bc_info;
int gmsx_betweenness(const gmsx_graph *g, int64_t n_sources, const int32_t *sources /* host */, uint32_t flags,
                     double *scores /* n, host */, gmsx_bc_info *info /* required */, gmsx_stats *stats);

/* ---- batched multi-source breadth-first search: closeness, harmonic centrality, eccentricity (no reference counterpart; msbfs.hip).
 * gmsx_bfs_multi runs a BFS from every listed source, bit-parallel: a vertex holds W 64-bit words, one bit per source, and the sources are
 * processed in passes of 64 W consecutive list entries (W: option MSBFS_WORDS), so one sweep of the CSR advances 64 W traversals.  A source listed
 * twice is two rows of `depth` and counts twice in dist_sum and reach, as gmsx_betweenness counts it.  The integer outputs do not depend on the
 * pass structure; closeness and harmonic are computed on the host from each source's per-level counts, ascending in the depth — every output is a
 * function of (graph, sources) alone, byte-identical in every run and under every MSBFS_* option, GMSX_UPLOAD_TRUSTED, GMSX_UPLOAD_HUB_LIMIT and
 * a sharded upload, except passes, push_levels and pull_levels, which are functions of (graph, sources, options).  On the undirected graphs this
 * library holds, with all n vertices as sources: dist_sum[v] is v's farness, far[v] its eccentricity inside its component, and
 * per_source[i].depth_sum == dist_sum[sources[i]].  A level is pushed (integer atomicOr only) or pulled (one owner per vertex) by the rule of
 * MSBFS_DIRECTION / MSBFS_ALPHA; push_levels + pull_levels counts the levels that found a vertex: Σ over the passes of the largest levels - 1.
 * NULL g or info, n_sources < 0, NULL sources with n_sources > 0, an id outside [0, n): GMSX_ERR_INVALID, nothing written.  n_sources = 0: GMSX_OK,
 * dist_sum and reach zeros, far -1, info zeroed.  A level count above n, a bounded append past its bound, or per-source sums that disagree with
 * the per-vertex sums (Σ_i reached_i == Σ_v reach[v], summed on the device): GMSX_ERR_KERNEL.  The caller's arrays are written only after the flag
 * words were read as zero, through host staging.  depth is optional and meant for tests and small graphs: the device holds one pass's rows
 * (256 W n bytes); if that does not fit: GMSX_ERR_DEVICE_MEM.  Single GPU, the source list is not sharded.  gmsx_stats: kernel_ms, setup_ms,
 * launches, units = Σ reached_arcs, probes = Σ over the passes of the pass's level count (its largest levels). */
typedef struct {
    int64_t reached;       /* as gmsx_bfs_info, for this source */
    int64_t reached_arcs;
    int64_t depth_sum;
    int32_t levels;
    int32_t reserved;
    double  closeness;     /* (reached - 1) / depth_sum, 0.0 when depth_sum == 0 */
    double  harmonic;      /* sum over d = 1 .. levels-1, ascending, of double(count_d) / double(d); count_d = vertices at depth d */
} gmsx_bfs_source;
typedef struct {
    int64_t sources, passes, reached_total;
    int32_t max_levels;    /* largest levels of any source */
    int32_t max_far;       /* largest depth met = max of far[] (a diameter lower bound; exact with every vertex as a source) */
    int32_t push_levels, pull_levels;   /* summed over the passes: facts about (graph, sources, options) */
} gmsx_bfs_multi_info;
int gmsx_bfs_multi(const gmsx_graph *g, int64_t n_sources, const int32_t *sources /* host */,
                   gmsx_bfs_source *per_source /* n_sources, host, or NULL */,
                   int32_t *depth    /* n_sources * n, row i = depths from sources[i], -1 unreachable; host, or NULL */,
                   int64_t *dist_sum /* n: sum over the listed sources that reach v of depth_i(v); host, or NULL */,
                   int32_t *reach    /* n: how many listed sources reach v; host, or NULL */,
                   int32_t *far      /* n: largest depth_i(v) over them, -1 if none; host, or NULL */,
                   gmsx_bfs_multi_info *info /* required */, gmsx_stats *stats);

/* ---- PageRank (gms/representations/graphs/log_graph/pr.cc: PageRankPull, PRVerifier; pagerank.hip), the reference's constants as arguments
 * (its own: damping 0.85, 20 sweeps, tolerance 1e-4).  t = teleport / Σ teleport (the host sums it ascending, in double), or 1 / n per entry when
 * teleport is NULL.  scores = t at the start; every sweep computes contrib[v] = scores[v] / deg(v), new[u] = (1 - damping) t[u] + damping
 * Σ_{v in N(u)} contrib[v] and error = Σ_u |new[u] - old[u]|; the loop stops behind the sweep whose error < tolerance, or after max_iters sweeps
 * (tolerance = 0 never stops early, max_iters = 0 returns t).  A vertex of degree 0 keeps (1 - damping) t[u] and its own mass is dropped, as the
 * reference drops it (so sum < 1 when such vertices exist); the device never divides by zero.  GMSX_PR_DANGLING hands that mass D = Σ_{deg(v) = 0}
 * old[v] back through t: new[u] += damping D t[u], and sum stays 1 up to rounding.  GMSX_PR_FLOAT32 holds scores and contributions as float, the
 * reference's ScoreT — every row sum and the error are still accumulated in double, and every value of `scores` is exactly a float; the default
 * is double throughout.  gmsx_pagerank_residual is PRVerifier (pr.cc:79-97) as a number: Σ_u |(1 - damping) t[u] + damping Σ contrib[v] (+ the
 * dangling term) - scores[u]| for one sweep over the caller's scores; nothing is stored; PRVerifier(g, s, tol) <=> residual < tol.
 * No floating-point atomic is used: a row's sum is taken by a rule that is a function of the row's length alone (pagerank.hip states it), and the
 * per-sweep error, sum and D are reduced over fixed blocks of vertices by a fixed tree — scores and every info field are byte-identical in every
 * run and process, under GMSX_UPLOAD_TRUSTED, GMSX_UPLOAD_HUB_LIMIT and a sharded upload.  NULL g, info or residual, NULL scores in
 * gmsx_pagerank_residual with n > 0, damping outside [0, 1] or NaN, max_iters < 0, a negative or NaN tolerance, a teleport with a negative, NaN
 * or infinite entry or with sum 0, unknown flag bits: GMSX_ERR_INVALID, nothing written.  n = 0: GMSX_OK, info zeroed (argmax = -1).  A bin list
 * that would overflow, a bin total that is not n, or a non-finite score: GMSX_ERR_KERNEL.  The caller's arrays are written only after the device
 * flag word was read as zero.  Single GPU, no shards.  gmsx_stats: kernel_ms (the sweeps), setup_ms (binning, teleport upload, final reductions),
 * launches, units = iterations * nnz, probes = iterations. */
enum { GMSX_PR_DEFAULT = 0, GMSX_PR_DANGLING = 1, GMSX_PR_FLOAT32 = 2 };
typedef struct {
    int32_t iterations;   /* sweeps executed (<= max_iters) */
    int32_t converged;    /* 1 iff the last sweep's error < tolerance */
    int32_t argmax;       /* vertex of the largest score; ties: the smallest id; -1 for n = 0 */
    int32_t reserved;
    double  error;        /* Σ_u |new[u] - old[u]| of the last sweep; 0.0 when iterations == 0 */
    double  sum;          /* Σ_u scores[u] */
    double  max_score;
    int64_t isolated;     /* vertices of degree 0 */
} gmsx_pagerank_info;
int gmsx_pagerank(const gmsx_graph *g, double damping, int32_t max_iters, double tolerance,
                  const double *teleport /* n, host, or NULL = uniform */, uint32_t flags,
                  double *scores /* n, host, or NULL */, gmsx_pagerank_info *info /* required */, gmsx_stats *stats);
int gmsx_pagerank_residual(const gmsx_graph *g, const double *scores /* n, host */, double damping,
                           const double *teleport, uint32_t flags, double *residual, gmsx_stats *stats);

/* ---- edge weights on the device and single-source shortest paths (gms/representations/graphs/log_graph/sssp.cc: DeltaStep, SSSPVerifier;
 * sssp.hip).
 * gmsx_graph_set_weights attaches weights[nnz] (host, parallel to the uploaded neighbour array) to a handle; NULL detaches.  Attachment is
 * explicit: gmsx_graph_upload_csr of a weighted CSR uploads the structure only.  The array is validated on the device: a weight below 1 →
 * GMSX_ERR_INVALID (never skipped; positive weights are what makes parent a tree and the verifier exact); weight(u→v) != weight(v→u) — the twin
 * found by a bounded binary search in v's row — → GMSX_ERR_NOT_CANONICAL, a check a handle uploaded with GMSX_UPLOAD_TRUSTED skips.  A failed
 * attach leaves the handle as it was; a second attach replaces the first.  The weights count in gmsx_graph_device_bytes and are released by
 * gmsx_graph_free.  No other entry point reads them.  gmsx_graph_has_weights: 1 / 0.
 * gmsx_sssp: dist[v] = the weight of a lightest path from source (dist[source] = 0; -1: unreachable); parent[v] = the SMALLEST-id neighbour u
 * with dist[u] + w(u,v) == dist[v], parent[source] = source, -1 for an unreachable vertex.  Weights are at least 1, so dist strictly falls along
 * parents: parent is a tree.  With all weights 1, dist and parent equal gmsx_bfs's depth and parent element for element.  The distances are
 * found by delta-stepping (bucket i = tentative distances in [i delta, (i + 1) delta); delta > 0: as given, 0: max(1, SSSP_DELTA_AUTO * mean
 * weight / mean degree)); parent by a PULL pass behind it — every reached vertex takes the first tight entry of its ascending row, one writer per
 * vertex, no atomics — which also checks the relaxation: a reached vertex without a tight entry → GMSX_ERR_KERNEL.  dist, parent and every info
 * field except rounds and relaxations are facts about (graph, weights, source) — buckets and delta about delta as well — byte-identical in
 * every run and process, under every delta, every SSSP_* option, GMSX_UPLOAD_TRUSTED, GMSX_UPLOAD_HUB_LIMIT and a sharded upload.  Distances
 * are held in 32-bit words when (n - 1) * wmax < 2^31 - 1, else in 64-bit words (info->wide).
 * No weights attached, source outside [0, n), NULL g or info, delta < 0: GMSX_ERR_INVALID, nothing written.  An append past its bound, more
 * than n + 1 rounds in one bucket (a bucket is done after at most n Bellman–Ford rounds) or more buckets than min(n, (n - 1) wmax / delta + 2):
 * GMSX_ERR_KERNEL.  The caller's arrays are written only after the flag words were read as zero.  Single GPU, no shards.  gmsx_stats:
 * kernel_ms, setup_ms, launches, units = reached_arcs, probes = buckets.
 * gmsx_sssp_verify is the same pull pass over a caller's array (an entry below 0 = unreached): violated_arcs = arcs u→v, both ends reached,
 * with dist[v] > dist[u] + w; untight = reached vertices other than the source without a tight arc; wrong_unreached = unreached vertices with
 * a reached neighbour; source_ok = 1 iff dist[source] == 0.  SSSPVerifier(g, source, dist) (sssp.cc:145-175) <=> all three counts are 0 and
 * source_ok is 1.  NULL g, dist (n > 0) or out, no weights, a bad source: GMSX_ERR_INVALID. */
int gmsx_graph_set_weights(gmsx_graph *g, const int32_t *weights /* nnz, host, parallel to the uploaded neigh; NULL detaches */);
int gmsx_graph_has_weights(const gmsx_graph *g);
typedef struct {
    int64_t reached, reached_arcs;   /* as gmsx_bfs_info */
    int64_t dist_sum, max_dist;      /* over the reached vertices */
    int64_t delta;                   /* the bucket width used */
    int64_t buckets;                 /* non-empty buckets = distinct dist[v] / delta over the reached vertices: a fact about (graph, weights, source, delta) */
    int64_t rounds, relaxations;     /* diagnostics: may differ between runs and under SSSP_* options */
    int32_t far_vertex;              /* smallest id at max_dist; the source if nothing else is reached */
    int32_t wide;                    /* 1 = 64-bit distance words were used */
} gmsx_sssp_info;
int gmsx_sssp(const gmsx_graph *g, int32_t source, int64_t delta /* > 0: as given; 0: the library's choice */,
              int64_t *dist /* n, host, or NULL; -1 = unreachable */, int32_t *parent /* n, host, or NULL */,
              gmsx_sssp_info *info /* required */, gmsx_stats *stats);
typedef struct { int64_t violated_arcs, untight, wrong_unreached; int32_t source_ok, reserved; } gmsx_sssp_check;
int gmsx_sssp_verify(const gmsx_graph *g, int32_t source, const int64_t *dist /* n, host */, gmsx_sssp_check *out, gmsx_stats *stats);

/* ---- minimum (or maximum) spanning forest over the attached weights (msf.hip; no reference counterpart, like the k-truss).
 * THE ORDER.  An edge is e = {u, v} with lo = min(u, v), hi = max(u, v) and weight w.  Minimum: key(e) = (w, lo, hi), compared
 * lexicographically.  Maximum (GMSX_MSF_MAXIMUM in flags): the heavier edge comes first, ties are still broken by the smaller (lo, hi).  The CSR
 * has no parallel edges and no self loops, so the order is strict, and the spanning forest under it is unique: "the forest" is Kruskal's output
 * under that order, which is also the output of Borůvka's rounds under it — what the device runs: in every round every current component that
 * has one picks its first crossing edge in the order, and all picks are applied (union_find.hpp's links: a root goes under a smaller id).
 * edge_u / edge_v / edge_w (all three or none): the forest's edges with edge_u[i] < edge_v[i], ascending by (u, v) — the CSR order of the u < v
 * arcs; the first info->edges entries are written.  arc_keep: a symmetric 0 / 1 byte per arc of the uploaded CSR, the shape gmsx_jarvis_patrick
 * produces and gmsx_connected_components consumes; exactly 2 * edges bytes are 1.  label[v] = the smallest vertex id of v's tree, which is
 * gmsx_connected_components(g, NULL)'s label byte for byte.  info->rounds counts the rounds that added an edge: the components after round r are
 * a fact about (graph, weights, flags), so rounds is, and rounds <= floor(log2(max(largest_tree, 1))).
 * Every output except the gmsx_stats times is byte-identical in every run and process, under every MSF_* option, GMSX_UPLOAD_TRUSTED,
 * GMSX_UPLOAD_HUB_LIMIT, a sharded upload and re-attached weights.
 * No weights attached, NULL g or info, unknown flag bits, only one or two of the three edge arrays: GMSX_ERR_INVALID, nothing written.  A walk
 * or retry past its cap (n + 64), an append past its bound, more than 64 rounds, a picked arc whose twin is not found (possible only under
 * GMSX_UPLOAD_TRUSTED), or an edge count that is not n - trees: GMSX_ERR_KERNEL.  The caller's arrays are written only after the flag word was
 * read as zero, through host staging.  Single GPU, no shards.  n = 0 or no edge: GMSX_OK with trees = isolated = n.  The handle is not modified;
 * the call's device state is O(n) words and one byte per arc.  Test hooks: options MSF_WAVE_ROW, MSF_WG_ROW (first guesses, not
 * tuned) and MSF_PRUNE.  gmsx_stats: kernel_ms (the rounds), setup_ms (buffers, the edge list and the info reduction), launches, units = edges, probes =
 * rounds, alg_elements = arcs the search pass examined. */
enum { GMSX_MSF_MAXIMUM = 1u };
typedef struct {
    int64_t edges;          /* forest edges = n - trees */
    int64_t total_weight;   /* sum of their weights */
    int64_t trees;          /* components of the graph, isolated vertices included */
    int64_t isolated;
    int64_t largest_tree;   /* vertices of the largest tree; 0 for n = 0 */
    int32_t min_weight, max_weight;  /* lightest / heaviest forest edge (the bottleneck); 0 when edges == 0 */
    int32_t rounds;         /* Boruvka rounds that added at least one edge: a fact about (graph, weights, flags) */
    int32_t reserved;
} gmsx_msf_info;
int gmsx_min_spanning_forest(const gmsx_graph *g, uint32_t flags,
                             int32_t *edge_u, int32_t *edge_v, int32_t *edge_w /* each: room for n - 1 entries, host, or NULL (all three or none) */,
                             uint8_t *arc_keep /* nnz, host, or NULL */, int32_t *label /* n, host, or NULL */,
                             gmsx_msf_info *info /* required */, gmsx_stats *stats);

/* ---- label-propagation communities and the exact modularity of a labelling (communities.hip; no reference counterpart).  Everything is an
 * integer; nothing on the device is floating point.
 * INPUTS.  The uploaded CSR and, with GMSX_LP_WEIGHTED in flags, the attached weights (>= 1, symmetric unless the handle was uploaded with
 * GMSX_UPLOAD_TRUSTED); without the flag every arc weighs 1.
 * COLOURING.  A proper colouring c[v] in 1 … C fixes the order of the work.  A caller's array is checked on the device: a colour below 1 or
 * above n, or an edge with equal colours at its ends → GMSX_ERR_INVALID, nothing written.  NULL = exactly the array gmsx_coloring_jp(g, NULL, …)
 * returns, computed by the same code and left on the device.
 * A SWEEP.  label[v] = v at the start.  The colours are taken in the order 1, 2, …, C, all vertices of a colour at once.  W_v(l) = the total
 * weight (an int64 sum) of v's arcs to neighbours that hold label l now, M = max_l W_v(l).  If W_v(label[v]) == M, v keeps its label (an
 * isolated vertex always does); otherwise it takes the SMALLEST l with W_v(l) == M.  A colour class is an independent set, so this is the
 * sequential asynchronous propagation that visits the vertices ascending by (colour, id) — the whole CPU restatement.
 * STOP.  After the first sweep that changes no label (converged = 1), or after max_sweeps sweeps (converged = 0 unless that last sweep changed
 * nothing); max_sweeps == 0: the library's cap of 1000; max_sweeps < 0: GMSX_ERR_INVALID.  Every change makes the vertex's label strictly
 * heavier among its neighbours and no neighbour moves at the same time, so under symmetric weights the total weight of the arcs whose ends share
 * a label rises strictly with every change and the propagation ends; asymmetric weights (TRUSTED) have only the cap.
 * gmsx_modularity scores any labelling with labels in [0, n): W = the total arc weight (2 m unweighted), I = the total weight of the arcs whose
 * ends share a label (both directions), D_c = the weighted degrees of the vertices labelled c, S = Σ_c D_c² exactly, in 128 bits (hi, lo).
 * modularity = I / W - S / W², computed once on the host by the fixed expression (long double)I / W - ((long double)hi * 2^64 + lo) / (W * W)
 * in long double and rounded to double; 0 when W = 0.  The integers are the contract, modularity is a convenience.  unstable = the non-isolated
 * vertices with W_v(label[v]) < M: a labelling is a fixed point of the propagation under every colouring iff unstable == 0.
 * label and every field of both info blocks are byte-identical in every run and process, under every LP_* option, GMSX_UPLOAD_TRUSTED,
 * GMSX_UPLOAD_HUB_LIMIT, a sharded upload, a second handle and re-attached weights; "smallest label" is the smallest in the caller's ids.
 * NULL g or info, unknown flag bits, GMSX_LP_WEIGHTED without attached weights, a NULL label (n > 0) or one outside [0, n) in gmsx_modularity:
 * GMSX_ERR_INVALID, nothing written.  n = 0: GMSX_OK, info zeroed.  No edge: n singletons, sweeps = 1, converged = 1, modularity = 0.  A table
 * insert or a placement past its bound, or a probe loop past its cap: GMSX_ERR_KERNEL; nothing is written out of bounds.  The caller's arrays
 * are written only after the device flag word was read as zero.  Single GPU, no shards; the handle is not modified.  Test hooks: options
 * LP_WAVE_ROW, LP_LDS_ROW, LP_LDS_SLOTS, LP_WG_WORK, LP_ACTIVE.  gmsx_stats: kernel_ms (the sweeps / the scoring pass), setup_ms, launches,
 * units = rows evaluated, alg_elements = arcs gathered, probes = sweeps — these may differ under the options. */
enum { GMSX_LP_WEIGHTED = 1u };
typedef struct {
    int64_t communities;   /* distinct labels at the end */
    int64_t largest;       /* vertices of the largest community */
    int64_t singletons;    /* communities of one vertex, isolated vertices included */
    int64_t changes;       /* label changes over all sweeps: a fact about (graph, weights, colouring, max_sweeps) */
    int64_t first_sweep_changes;
    int32_t sweeps;        /* sweeps run, the changeless last one included */
    int32_t colors;        /* C */
    int32_t converged, largest_label;   /* ties: the smallest label */
} gmsx_lp_info;
int gmsx_label_propagation(const gmsx_graph *g, uint32_t flags, const int32_t *coloring /* n, host, or NULL */, int32_t max_sweeps,
                           int32_t *label /* n, host, or NULL */, gmsx_lp_info *info /* required */, gmsx_stats *stats);
typedef struct {
    int64_t total_weight, intra_weight;   /* W, I */
    uint64_t sumsq_hi, sumsq_lo;          /* S */
    int64_t communities, largest, unstable;
    double modularity;
} gmsx_modularity_info;
int gmsx_modularity(const gmsx_graph *g, uint32_t flags, const int32_t *label /* n, host */, gmsx_modularity_info *info /* required */,
                    gmsx_stats *stats);

/* ---- greedy (weighted) matching and its verifier (matching.hip; no reference counterpart, like the k-truss and the spanning forest).
 * THE ORDER.  An edge is e = {lo, hi}, lo < hi, with weight w: the attached weight (in [1, 2^31 - 1]) with GMSX_MATCH_WEIGHTED in flags, else
 * w = 1 for every edge, and no weights need be attached.  key(e) = (heavier w first, h(lo, hi) ascending, lo ascending, hi ascending), h a
 * fixed 32-bit mixer in uint32 arithmetic:
 *     h = lo * 0x9E3779B1 + hi;  h ^= h >> 16;  h *= 0x85EBCA6B;  h ^= h >> 13;  h *= 0xC2B2AE35;  h ^= h >> 16;
 * (h(0,1) = 0x514e28b7, h(0,2) = 0x30f4c306, h(1,2) = 0x7e32275d, h(5,7) = 0xc71f3556).  The CSR has no parallel edges and no self loops,
 * so the trailing (lo, hi) makes the order strict.  The hash is in the order because plain (lo, hi) ties serialise the rounds below (a path
 * of unit weights takes n / 2 rounds without it, 3 with it); two arcs of one row can share h — h(0, 50549) =
 * h(50549, 62096) = 0xe935fad8 —, so the tail does decide.
 * "THE MATCHING" is the output of the sequential greedy algorithm: take the edges in the order and keep an edge iff both ends are still free.
 * It is a maximal matching; with weights its total weight is at least half the maximum's.  The device runs the locally dominant rounds
 * (Preis; Manne, Bisseling), which give the same matching: vertex v is LIVE while it is free and has a free neighbour; in a round every live
 * v finds cand[v], the other end of the first arc of its row in the order whose other end is free (none: v is dead for good, matched
 * vertices stay matched), then mate[v] = cand[v] wherever cand[cand[v]] == v; until no vertex is live.  The first live edge in the order is
 * always mutual, so every round matches at least one edge and rounds <= pairs <= n / 2; the set matched in round r is the set of locally
 * dominant edges among the live ones, so info->rounds (the rounds that matched an edge) is a fact about (graph, weights, flags) like
 * everything else.  A path with strictly increasing weights takes one round per pair: that is inherent in the order.
 * mate[v] = v's partner or -1 (free).  edge_u / edge_v / edge_w (all three or none, room for n / 2 entries each): the pairs with
 * edge_u[i] < edge_v[i], ascending by u, and their weights (1 when unweighted); the first info->pairs entries are written.
 * Every output except gmsx_stats is byte-identical in every run and process, under every MATCH_* option, GMSX_UPLOAD_TRUSTED,
 * GMSX_UPLOAD_HUB_LIMIT, a sharded upload (the call is single-GPU and reads the whole CSR) and re-attached weights.
 * NULL g or info, unknown flag bits, GMSX_MATCH_WEIGHTED without attached weights, one or two of the three edge arrays: GMSX_ERR_INVALID,
 * nothing written.  n = 0 or no edge: GMSX_OK, pairs = 0, rounds = 0, every vertex free.  An append past its bound, more than n / 2 + 1
 * rounds, or a failed check of the result (2 * pairs != matched vertices, a mate whose mate is someone else, a live vertex left):
 * GMSX_ERR_KERNEL.  The caller's arrays are written only after the flag word was read as zero, through host staging.  The handle is not
 * modified; the call's device state is O(n) words.  Test hooks: options MATCH_WAVE_ROW, MATCH_WG_ROW (first guesses, not tuned) and
 * MATCH_KEEP.  gmsx_stats: kernel_ms (the rounds), setup_ms (buffers, the edge list and the info reduction), launches, units = pairs,
 * probes = rounds, alg_elements = arcs the search pass examined (may differ under the options).
 * gmsx_matching_verify: the six integers of gmsx_matching_check for any mate array under the same flags.  A vertex is INVALID if its
 * mate is outside [-1, n), is itself or no neighbour, or if its mate's mate is not the vertex; the other fields treat invalid vertices as
 * free (pairs, total_weight over the valid pairs; free_vertices = n - 2 * pairs).  THE CERTIFICATE: invalid == 0 && undominated == 0 holds
 * iff mate is THE greedy matching under the order (induction over the order: an edge greedy keeps has no earlier adjacent matching edge, so
 * it must be in the matching; an edge greedy rejects has one, so it cannot be) — an O(m) check that needs no second run.  Every augmentable
 * edge is also undominated.  NULL g or out, NULL mate with n > 0, unknown flag bits, GMSX_MATCH_WEIGHTED without weights: GMSX_ERR_INVALID. */
enum { GMSX_MATCH_WEIGHTED = 1u };
typedef struct {
    int64_t pairs, total_weight;      /* total_weight = pairs when unweighted */
    int64_t free_vertices, exposed;   /* unmatched; unmatched with degree >= 1 (all their neighbours are matched) */
    int32_t min_weight, max_weight;   /* over the matched edges; 0 when pairs == 0 */
    int32_t rounds, reserved;
} gmsx_matching_info;
int gmsx_greedy_matching(const gmsx_graph *g, uint32_t flags, int32_t *mate /* n, host, or NULL; -1 = free */,
                         int32_t *edge_u, int32_t *edge_v, int32_t *edge_w /* room for n / 2 each, all three or none; u < v, ascending by u */,
                         gmsx_matching_info *info /* required */, gmsx_stats *stats);
typedef struct {
    int64_t invalid;       /* vertices whose mate is outside [-1, n), is not a neighbour, or whose mate's mate is not them */
    int64_t pairs, total_weight, free_vertices;   /* over the valid pairs */
    int64_t augmentable;   /* edges with both ends free: the matching is maximal iff 0 */
    int64_t undominated;   /* non-matching edges with no adjacent matching edge EARLIER in the order */
} gmsx_matching_check;
int gmsx_matching_verify(const gmsx_graph *g, uint32_t flags, const int32_t *mate /* n, host */, gmsx_matching_check *out, gmsx_stats *stats);

/* ---- biconnected components, articulation points and bridges (bicc.hip; no reference counterpart, like the k-truss and the spanning
 * forest).
 * BLOCKS.  A block (biconnected component) is a maximal set of edges in which any two edges lie on a common simple cycle; a BRIDGE is a
 * block of one edge.  Every edge lies in exactly one block.  BLOCK IDS are dense, 0 … blocks - 1, and ascend with each block's smallest edge
 * under the order (min end, max end) — the CSR order of the `u < v` arcs; they fit 32 bits because blocks <= n - components.
 * block[j] = the id of the block of edge {u, neigh[j]}, parallel to the uploaded neigh: both arcs of an edge carry the same id.
 * blocks_at[v] = the number of blocks that contain v, 0 for an isolated vertex; v is an ARTICULATION POINT (cut vertex) iff blocks_at[v] >= 2.
 * arc_keep[j] = 0 for a bridge, else 1: symmetric, the shape gmsx_jarvis_patrick and gmsx_min_spanning_forest produce; fed to
 * gmsx_connected_components it gives the 2-edge-connected components.
 * levels = the non-empty levels of the BFS forest rooted at every component's smallest id: the roots are fixed and BFS depth is unique, so
 * it is a fact about the graph.
 * ALWAYS: Σ blocks_at = n - components + blocks; the components over arc_keep = components + bridges; Σ over the blocks of their edges =
 * nnz / 2.
 * The device runs Tarjan–Vishkin on a BFS forest (integers only): component roots by the union-find, a forest by claims, subtree sizes,
 * preorder numbers, low and high by three sweeps over the levels, a second union-find over the tree edges, then ids by the rank of each
 * set's first arc.  The forest depends on the arrival of the claims; the partition of the edges it yields does not.
 * Every output except the times of gmsx_stats is byte-identical in every run and process, under every BCC_* option, GMSX_UPLOAD_TRUSTED,
 * GMSX_UPLOAD_HUB_LIMIT, a sharded upload (the call is single-GPU and reads the whole CSR) and a second handle.
 * NULL g or info, unknown flag bits (flags must be 0): GMSX_ERR_INVALID, nothing written.  n = 0 or no edge: GMSX_OK, zeros, components =
 * isolated = n.  A capped walk exceeded (n + 64, union_find.hpp), an append past its bound, arcs without their twins (as many `u > v` as
 * `u < v` arcs are required; possible only under GMSX_UPLOAD_TRUSTED), or a failed self-check (order short of n vertices, Σ subtree sizes of
 * the roots != n, Σ edges of the sets != nnz / 2, the first identity on the device's own numbers): GMSX_ERR_KERNEL.  The caller's arrays
 * are written only after the flag word was read as zero, through host staging.  The handle is not modified; the call's device state is O(n)
 * words, plus 4 bytes per arc for block and 1 byte per arc for arc_keep only when the caller asks for them.  Test hooks: options
 * BCC_WAVE_ROW, BCC_WG_ROW, BCC_WG_FRONTIER, BCC_WG_LEVEL (first guesses, not tuned).  gmsx_stats: kernel_ms (the kernels), setup_ms (buffers
 * and the copies back), launches, units = blocks, probes = levels, alg_elements = arcs the arc passes examined. */
typedef struct {
    int64_t blocks;                 /* biconnected components (bridges are blocks of one edge); 0 without edges */
    int64_t bridges;                /* blocks of exactly one edge */
    int64_t articulation_points;    /* vertices with blocks_at >= 2 */
    int64_t largest_block_edges;    /* edges of the largest block (by edges) */
    int64_t largest_block_vertices; /* its vertices */
    int64_t components;             /* connected components, isolated vertices included */
    int64_t isolated;
    int32_t largest_block;          /* its id; ties: the smallest id */
    int32_t max_blocks_at;          /* largest blocks_at[v] */
    int32_t levels;                 /* non-empty levels of the BFS forest rooted at every component's smallest id */
    int32_t reserved;
} gmsx_bicc_info;
int gmsx_biconnected_components(const gmsx_graph *g, uint32_t flags /* 0 */, int32_t *block /* nnz, host, or NULL */,
                                int32_t *blocks_at /* n, host, or NULL */, uint8_t *arc_keep /* nnz, host, or NULL */,
                                gmsx_bicc_info *info /* required */, gmsx_stats *stats);

/* ---- 4-cycle counting and the 3- / 4-vertex motif census.  No reference counterpart (like the k-truss: a member of the family the suite
 * describes and does not build).  All results are exact integers.
 * gmsx_cycle4_count: *cycles = the 4-cycles of the graph (subgraphs, not necessarily induced; the butterflies of a bipartite graph).
 * at_vertex[v] (n entries, indexed by the vertex ids of the uploaded CSR; may be NULL) = the 4-cycles through v = Σ_{w != v} C(|N(v) ∩ N(w)|, 2);
 * their sum is 4 * *cycles.  THE RULE (motifs.hip): in the device's rank ids (decreasing (degree, id), rank 0 = the biggest hub) a cycle is
 * counted once, at its vertex u of the smallest rank id, against the opposite vertex w — a WEDGE is a path u - v - w with rank(v) > rank(u) and
 * rank(w) > rank(u), and the cycles of u are Σ_w C(wedges from u to w, 2).  A source with fewer than two later neighbours is not walked.
 * gmsx_cycle4_partial: the cycles whose source belongs to shard `part` of `nparts` — a shard is a set of whole sources, assigned by the rule of
 * gmsx_tc_partial applied to the source's rank id; the partials of one nparts add up to *cycles; (0, 1) is the whole graph, other out-of-range
 * pairs → GMSX_ERR_INVALID.  No at_vertex in a partial.
 * gmsx_motif_census4 (single GPU): subgraphs[] = non-induced copies (a copy = a vertex subset and an edge subset isomorphic to the motif, each
 * once), induced[] = vertex subsets whose induced subgraph IS the motif.  With d the degree, sup(e) the support of gmsx_edge_support, T the
 * triangles: wedge = Σ_v C(d_v, 2); star3 = Σ_v C(d_v, 3); triangle = Σ_e sup(e) / 3; path4 = Σ_{e = {u,v}} (d_u - 1)(d_v - 1) - 3 T;
 * paw (tailed triangle) = ½ Σ_e sup(e)(d_u + d_v - 4); diamond = Σ_e C(sup(e), 2); clique4 = gmsx_kclique_count(k = 4); cycle4 = the kernel
 * above.  Induced: I_K4 = K4; I_diamond = diamond - 6 K4; I_C4 = cycle4 - I_diamond - 3 K4; I_paw = paw - 4 I_diamond - 12 K4; I_star3 =
 * star3 - I_paw - 2 I_diamond - 4 K4; I_path4 = path4 - 2 I_paw - 4 I_C4 - 6 I_diamond - 12 K4; I_triangle = T; I_wedge = wedge - 3 T.
 * The sums are finished in 128 bits on the host: if any non-induced count does not fit 64 bits the call returns GMSX_ERR_OVERFLOW and writes
 * nothing (Σ C(d, 3) alone passes 2^64 on a star of 4.9 M leaves).  The 4-cycle calls return GMSX_ERR_OVERFLOW, too, when wedges_walked *
 * max_codegree / 2 — a bound of their 64-bit sum — does not fit 64 bits (more than 2^34 wedges at the least).
 * n = 0 or no edge: GMSX_OK and zeros.  NULL g, info or cycles: GMSX_ERR_INVALID.  Outputs are written only after the device flag word was read
 * as zero; a counter index outside its span, or a harvest that disagrees with the wedges counted (a counter that was not zero before or after
 * its source), → GMSX_ERR_KERNEL; nothing is written out of bounds.  Every output except the gmsx_stats times is byte-identical in every
 * process and run.  Test hooks: options C4_LDS_SPAN, C4_SLAB_MB, C4_SPLIT_WEDGES.  gmsx_stats: kernel_ms (the wedge kernels), setup_ms (source
 * binning and the counter spans; census: also the support pass, the reductions and the 4-clique count), launches, units = sources walked,
 * alg_elements = wedges_walked. */
enum { GMSX_MOTIF_WEDGE = 0, GMSX_MOTIF_TRIANGLE = 1, GMSX_MOTIF_STAR3 = 2, GMSX_MOTIF_PATH4 = 3,
       GMSX_MOTIF_PAW = 4, GMSX_MOTIF_CYCLE4 = 5, GMSX_MOTIF_DIAMOND = 6, GMSX_MOTIF_CLIQUE4 = 7, GMSX_MOTIF_KINDS = 8 };
typedef struct {
    uint64_t subgraphs[GMSX_MOTIF_KINDS];  /* non-induced copies: vertex subsets times edge subsets, each copy once */
    uint64_t induced[GMSX_MOTIF_KINDS];    /* vertex subsets whose induced subgraph IS the motif */
    uint64_t wedges_walked;                /* wedges the 4-cycle kernels examined (diagnostic, a fact about the graph) */
    int32_t  max_codegree;                 /* largest counter value met: max over counted pairs (u, w) of |N(u) ∩ N(w)| restricted to later middles */
    int32_t  reserved;
} gmsx_motif_info;
int gmsx_cycle4_count(const gmsx_graph *g, uint64_t *cycles, int64_t *at_vertex /* n, host, or NULL */, gmsx_stats *stats);
int gmsx_cycle4_partial(const gmsx_graph *g, int part, int nparts, uint64_t *partial, gmsx_stats *stats);
int gmsx_motif_census4(const gmsx_graph *g, gmsx_motif_info *info /* required */, gmsx_stats *stats);

/* ---- the one collective of the path: the OpenMP reduction(+:total) of parallel/total.h:12,
 * k_clique_count_set_based.h:25 and the BK_CLIQUE_COUNTER atomic (tomita.h:76-77) across GPUs = ONE all-reduce of a u64 over
 * RCCL/xGMI.  One process per GPU; the 128-byte id is created on one rank (gmsx_comm_unique_id) and handed to the others by the
 * launcher (file, environment, MPI, torch.distributed store — the library does not care).  librccl is loaded on first use. */
typedef struct gmsx_comm gmsx_comm;
#define GMSX_COMM_ID_BYTES 128
int gmsx_comm_unique_id(void *id /* GMSX_COMM_ID_BYTES, out */);
/* ncclCommInitRank on the bound device, with a BOUNDED wait: the call runs on a helper thread and the caller waits at most GMSX_COMM_TIMEOUT_S
 * seconds (environment, default 180) for it — a peer that died or never started makes ncclCommInitRank wait for good.  GMSX_ERR_TIMEOUT then:
 * the helper thread stays parked inside RCCL, so the caller should report the failure and LEAVE THE PROCESS (its launcher — torch.distributed.run,
 * gmsx_driver's supervisor — takes the other ranks down).  The wait for the result of every gmsx_comm_allreduce_u64 is bounded the same way. */
int gmsx_comm_init(int rank, int nranks, const void *id /* GMSX_COMM_ID_BYTES */, gmsx_comm **out);
int gmsx_comm_allreduce_u64(gmsx_comm *c, uint64_t *value /* in: this rank's partial, out: the sum */); /* ncclAllReduce(count=1, ncclUint64, ncclSum) */
int gmsx_comm_rank(const gmsx_comm *c);
int gmsx_comm_size(const gmsx_comm *c);
int gmsx_comm_finalize(gmsx_comm *c);

#ifdef __cplusplus
}
#endif
#endif /* GMSX_H */
