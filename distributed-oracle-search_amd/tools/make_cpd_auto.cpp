// bin/make_cpd_auto — drop-in for warthog's make_cpd_auto (README.md:82-95),
// launched per worker by make_cpds.py:20-21:
//
//   make_cpd_auto --input X.xy --partmethod {div|mod} --partkey K
//                 --workerid I --maxworker W --outdir D
//                 [--partition M]      README.md:89 spelling of --partmethod
//                 [--device G]         default: I % (visible GPUs)
//                 [--batch B]          rows per GPU sweep (multiple of 1024);
//                                      0 (default) = what fits in HBM, at most
//                                      2048 rows when files are written (the
//                                      disk bounds the worker) and
//                                      28672 with --discard (CPD_BATCH_MAX
//                                      overrides), with or without the arena
//                 [--no-arena]         allocate the batch buffers at graph setup
//                                      instead of committing them on a host
//                                      thread beside the plan (default)
//                 [--arena-touch]      also write the arena once while committing
//                 [--threads T]        host threads for the hierarchy build (--ch-host)
//                 [--ch-host]          contract the hierarchy on host threads, not the GPU
//                 [--plan P | --no-plan-cache]
//                 [--write-threads T]  host threads copying + writing rows (16)
//                 [--no-pipeline]      build, then export, then write, per group
//                 [--plan-only]        build / load the cached plan and exit
//                 [--targets-from S]   only rows of targets of scenario S (q s t)
//                 [--format moves|rle] bucket file layout: moves (default) =
//                                      the rows as move tables of 1/2/4 bits
//                                      per column (by max out-degree, n*bits/8
//                                      bytes per row); rle = DOSCPD01, the run
//                                      words (4 B per run)
//                 [--stripes K]        moves: the rows striped over K part
//                                      files per bucket (DOSCPD03, default 16:
//                                      writes to one file serialise on its
//                                      inode); 1 = one DOSCPD02 file
//                 [--discard]          null sink: every row is still built and
//                                      copied out of HBM (D2H), but no file is
//                                      written (times the build + export path
//                                      without the disk); not with --no-pipeline
//                 [--hbm-reserve GIB]  HBM the automatic batch leaves to what
//                                      shares this GPU (a fifo_auto serving
//                                      beside the build)
//                 [--verbose]          the hierarchy build reports its rounds
//
// The plan (column order + hierarchy) is cached in D per graph; workers that
// start together share it through cpd_plan_cache (one builds, the rest wait).
//
// Builds the CPD rows of every target this worker owns under the
// distribution_controller partition, on the GPU, and writes one file per
// owned bucket into D (README.md:92-93 "one or more CPDs ... auto-generated
// names").  The launcher is fire-and-forget (tmux, make_cpds.py:21), so timing
// is printed here.
#include <sys/stat.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <deque>
#include <exception>
#include <functional>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "cli.hpp"
#include "cpd_io.hpp"

using cpd::io::CpdBucket;

static double now() {
    using namespace std::chrono;
    return duration<double>(steady_clock::now().time_since_epoch()).count();
}

static std::string dir_of(const std::string& p) {
    size_t s = p.find_last_of('/');
    return s == std::string::npos ? "." : p.substr(0, s);
}

static void ok(int rc, const char* what) {
    if (rc != CPD_OK)
        throw std::runtime_error(std::string(what) + " failed (" + std::to_string(rc) + "): " + cpd_last_error());
}

// ---- options ---------------------------------------------------------------

// Everything read from argv; the values are in the ranges parse_options checks.
struct Options {
    std::string input, method, outdir, format;
    std::string plan;    // "": <outdir>/<graph>.<fingerprint>.plan
    std::string device;  // "": worker id modulo the devices
    std::string targets_from;
    long long key = -1, wid = -1, W = -1;
    int mcode = 0, threads = 0, write_threads = 16;
    uint32_t stripes = 16, batch = 0, batch_cap = 2048;
    double hbm_reserve = 0.0;  // bytes
    bool moves = true, reserve_set = false, only_targets = false, discard = false;
    bool pipeline = true, plan_only = false, plan_cache = true;
    bool arena = true, arena_touch = false, ch_host = false, verbose = false;
};

static const char kUsage[] =
    "usage: make_cpd_auto --input X.xy --partmethod|--partition {div|mod} --partkey K "
    "--workerid I --maxworker W [--outdir D] [--device G] [--batch B] [--no-arena] "
    "[--arena-touch] [--threads T] [--ch-host] [--plan P | --no-plan-cache] "
    "[--write-threads T] [--no-pipeline] [--plan-only] [--targets-from SCEN] "
    "[--format moves|rle] [--stripes K] [--discard] [--hbm-reserve GIB] [--verbose]\n";

// How every check below refuses: its text on stderr, the exit status given.
static int refuse(int status, const char* text) {
    std::fputs(text, stderr);
    return status;
}

// Fills `o` from argv.  The checks run in this order, before anything is read
// or made; returns the exit status of the first that fails, or -1 to go on.
static int parse_options(int argc, char** argv, Options& o) {
    cli::Args a(argc, argv);
    o.input = a.str("input");
    o.method = a.str_any({"partmethod", "partition"});
    o.key = a.num("partkey", -1), o.wid = a.num("workerid", -1), o.W = a.num("maxworker", -1);
    if (o.input.empty() || o.method.empty() || o.key <= 0 || o.wid < 0 || o.W <= 0 || o.wid >= o.W)
        return refuse(2, kUsage);
    o.mcode = cli::method_code(o.method);
    o.format = a.str("format", "moves");
    if (o.format != "moves" && o.format != "rle")
        return refuse(2, "make_cpd_auto: --format must be moves or rle\n");
    o.moves = o.format == "moves";
    // compact buckets striped over part files (DOSCPD03; 1 = one DOSCPD02 file)
    const long long stripes = a.num("stripes", 16);
    if (stripes < 1 || stripes > 4096)  // what the reader accepts
        return refuse(2, "make_cpd_auto: --stripes must be in [1, 4096]\n");
    o.stripes = (uint32_t)stripes;
    o.discard = a.has("discard");
    o.pipeline = !a.has("no-pipeline");
    if (o.discard && !o.pipeline)
        return refuse(1, "make_cpd_auto: --discard needs the pipelined writer\n");
    // the automatic batch's cap, the same with or without the arena: writing
    // files, the sink bounds the worker (the GPU builds rows ~30x faster than
    // a disk takes them), so a batch past 2048 rows only adds HBM
    // to commit beside the plan; --discard keeps the build-bound cap
    const char* bm = std::getenv("CPD_BATCH_MAX");
    const double k1024 = bm && *bm ? std::max(1.0, std::min(32.0, std::floor(std::atof(bm) / 1024)))
                                   : o.discard ? 28.0 : 2.0;
    o.batch_cap = (uint32_t)k1024 * 1024u;
    o.batch = (uint32_t)a.num("batch", 0);
    o.outdir = a.str("outdir", dir_of(o.input));
    o.plan = a.str("plan");
    o.device = a.str("device");
    o.only_targets = a.has("targets-from");
    o.targets_from = a.str("targets-from");
    o.threads = (int)a.num("threads", 0);
    o.write_threads = (int)a.num("write-threads", 16);
    o.reserve_set = a.has("hbm-reserve");
    o.hbm_reserve = a.real("hbm-reserve", 0.0) * (double)(1ull << 30);
    o.plan_only = a.has("plan-only");
    o.plan_cache = !a.has("no-plan-cache");
    o.arena = !a.has("no-arena");
    o.arena_touch = a.has("arena-touch");
    o.ch_host = a.has("ch-host");
    o.verbose = a.has("verbose");
    return -1;
}

// ---- what the worker owns --------------------------------------------------

// The graph and this worker's share of its rows under the
// distribution_controller partition; `o` outlives it.
struct Work {
    const Options& o;
    const cpd::io::XYGraph g;
    uint64_t fp = 0;      // the graph's fingerprint
    uint32_t maxdeg = 1;  // largest out-degree: sizes the batch and the move width
    std::vector<uint32_t> owned;  // bucket ids
    // --targets-from SCEN: only the rows some query of the scenario needs
    // (its "q s t" targets; process_query.py:56-57 routes by t), so a
    // partial CPD for a known workload stays small on disk.  Empty: every row.
    std::vector<char> wanted;

    explicit Work(const Options& opts) : o(opts), g(cpd::io::read_xy(opts.input)) {
        fp = cpd::io::graph_fingerprint(g.n, g.row_ptr.data(), g.dst.data(), g.w.data());
        for (uint32_t v = 0; v < g.n; ++v) maxdeg = std::max(maxdeg, g.row_ptr[v + 1] - g.row_ptr[v]);
    }
    void list_owned() {
        uint32_t nb = 0;
        cli::check(cpd_partition_nbuckets(g.n, o.mcode, (uint32_t)o.key, &nb), "buckets");
        for (uint32_t b = 0; b < nb; ++b)
            if (b % (uint32_t)o.W == (uint32_t)o.wid) owned.push_back(b);
        if (!o.only_targets) return;
        wanted.assign(g.n, 0);
        for (const auto& q : cpd::io::read_scen(o.targets_from)) {
            if (q.second >= g.n) throw std::runtime_error("scenario target out of range");
            wanted[q.second] = 1;
        }
    }
    std::vector<uint32_t> bucket_nodes(uint32_t b) const {
        std::vector<uint32_t> v;
        auto keep = [&](uint64_t x) {
            if (wanted.empty() || wanted[x]) v.push_back((uint32_t)x);
        };
        if (o.mcode == CPD_PART_MOD) {
            for (uint64_t x = b; x < g.n; x += (uint64_t)o.key) keep(x);
        } else {
            const uint64_t chunk = ((uint64_t)g.n + o.key - 1) / o.key;
            for (uint64_t x = b * chunk; x < std::min<uint64_t>(g.n, (b + 1) * chunk); ++x) keep(x);
        }
        return v;
    }
    // bits per column of a move table (what the library packs the rows to)
    uint32_t move_bits() const { return maxdeg <= 2 ? 1u : maxdeg <= 4 ? 2u : 4u; }
    std::string path(uint32_t b) const {
        return cpd::io::bucket_path(o.outdir, o.input, o.method, (uint32_t)o.key, b);
    }
    // The header of bucket b with its targets (offsets and runs left empty).
    CpdBucket head(uint32_t b) const {
        CpdBucket h;
        h.n = g.n;
        h.bid = b;
        h.method = (uint32_t)o.mcode;
        h.key = (uint32_t)o.key;
        h.maxworker = (uint32_t)o.W;
        h.fingerprint = fp;
        h.targets = bucket_nodes(b);
        return h;
    }
    // The same header for a compact bucket of `words` words of `bits` bits per row.
    static cpd::io::MoveBucket move_head(const CpdBucket& h, uint32_t bits, uint32_t words) {
        cpd::io::MoveBucket m;
        m.n = h.n;
        m.bid = h.bid;
        m.method = h.method;
        m.key = h.key;
        m.maxworker = h.maxworker;
        m.bits = bits;
        m.words = words;
        m.fingerprint = h.fingerprint;
        m.targets = h.targets;
        return m;
    }
};

// Disk preflight: every owned row's bucket files must fit --outdir before the
// plan and the GPU work start (eight `div 8` workers of the 1M graph write
// 250 GB at once; a full disk would otherwise surface as a write error
// minutes in).  The rle layout's size depends on the runs, unknown before the
// build: not checked.  Returns 3 after its one line on stderr, or -1 to go on.
static int preflight(const Options& o, const Work& w) {
    if (!o.moves || o.discard || o.plan_only) return -1;
    uint64_t nrows = 0, need = 0, have = 0;
    for (uint32_t b : w.owned) nrows += w.bucket_nodes(b).size();
    cli::check(cpd_bucket_bytes(w.g.n, w.move_bits(), nrows, (uint32_t)w.owned.size(), o.stripes, &need),
               "bucket bytes");
    if (cpd_space_check(o.outdir.c_str(), need, &have) == CPD_OK) return -1;
    std::fprintf(stderr, "make_cpd_auto: %s\n", cpd_last_error());
    return 3;
}

// ---- device, plan and graph ------------------------------------------------

// --batch 0: the rows that fit in 85% of the free HBM above --hbm-reserve and
// `margin`, in steps of 1024 and at most the cap.  Less than one step: an
// error when `must_fit`, else 0, which leaves the batch to the library.
static uint32_t auto_batch(const Options& o, const Work& w, int device, double margin, bool must_fit) {
    uint64_t fr = 0, tot = 0, per1k = 0;
    cli::check(cpd_device_mem_info(device, &fr, &tot), "device memory");
    cli::check(cpd_batch_bytes(w.g.n, w.maxdeg, 1024, &per1k), "batch bytes");
    const double avail = (double)fr - o.hbm_reserve - margin;
    const double fit = avail > 0 ? std::floor(0.85 * avail / (double)per1k) : 0.0;
    if (fit < 1.0 && must_fit)
        throw std::runtime_error("HBM reserve leaves too little for a 1024-row batch");
    return fit < 1.0 ? 0u : (uint32_t)std::min((double)(o.batch_cap / 1024u), fit) * 1024u;
}

// The build's HBM (batch buffers and two move-table row sets) committed as an
// arena (cpd_device_arena) on a host thread while the plan is contracted or
// loaded: committing 100-200 GB takes seconds.  Joined by wait(), or on the
// way out.  Not committed: the library allocates at cpd_graph_set_batch.
struct ArenaStart {
    uint64_t bytes = 0;
    int rc = CPD_OK;
    std::string err;
    double seconds = 0.0, waited = 0.0;  // the commit; what wait() waited for it
    std::thread thr;
    ~ArenaStart() {
        if (thr.joinable()) thr.join();
    }
    void start(int device, uint64_t nbytes, bool touch) {
        bytes = nbytes;
        thr = std::thread([this, device, touch] {
            const double ta = now();
            rc = cpd_device_arena(device, bytes, touch ? 1 : 0);
            if (rc != CPD_OK) err = cpd_last_error();
            seconds = now() - ta;
        });
    }
    void wait() {
        if (!thr.joinable()) return;
        const double tw = now();
        thr.join();
        waited = now() - tw;
        if (rc != CPD_OK)
            std::fprintf(stderr, "make_cpd_auto: HBM arena not committed (%s)\n", err.c_str());
    }
    double gigabytes() const { return rc == CPD_OK ? bytes / 1e9 : 0.0; }
};

// The library handles of a run; released on every way out of main.
struct Session {
    cpd_plan* plan = nullptr;
    cpd_graph* dg = nullptr;
    cpd_rows* rows = nullptr;  // the sequential writer's
    int ndev = 0, device = -1;
    uint32_t batch = 0;  // rows per GPU sweep asked for (0: the library's default)
    bool arena = false;  // an ArenaStart was started on `device`
    Session() = default;
    Session(const Session&) = delete;
    ~Session() { release(); }
    // rows, graph, plan, then the arena (it must hold no live buffer); returns
    // what the arena's release returned
    int release() {
        cpd_rows_free(rows);
        cpd_graph_free(dg);
        cpd_plan_free(plan);
        rows = nullptr, dg = nullptr, plan = nullptr;
        const int rc = arena ? cpd_device_arena_release(device) : CPD_OK;
        arena = false;
        return rc;
    }
};

// The phases main times, in seconds (start: the clock at the first of them).
struct Phases {
    double start = 0, read = 0, plan = 0, graph = 0, batch_alloc = 0, setup = 0, rows = 0, free = 0;
    bool plan_loaded = false;
};

// Picks the device, starts the arena beside the plan, and makes the plan: host
// preprocessing (column order + hierarchy), cached per graph.
static void make_plan(const Options& o, const Work& w, Session& s, ArenaStart& arena, Phases& t) {
    const cpd::io::XYGraph& g = w.g;
    char fph[32];
    std::snprintf(fph, sizeof fph, "%016llx", (unsigned long long)w.fp);
    const std::string plan_path =
        o.plan.empty() ? o.outdir + "/" + cpd::io::xy_stem(o.input) + "." + fph + ".plan" : o.plan;
    const double t0 = now();
    cli::check(cpd_device_count(&s.ndev), "device count");
    if (s.ndev) s.device = (int)(o.device.empty() ? o.wid % s.ndev : std::atoll(o.device.c_str()));
    cpd_plan_opts po{};
    po.threads = o.threads;
    po.verbose = o.verbose;
    // the hierarchy is contracted on this worker's GPU (the same hierarchy
    // as the host build's, in a fraction of its time); --ch-host: threads
    po.ch_gpu = s.ndev > 0 && !o.ch_host;
    po.ch_device = std::max(s.device, 0);
    s.batch = o.batch;
    if (s.ndev > 0 && !o.plan_only && o.arena) {
        // beside the GPU contraction: a margin for its working set
        if (s.batch == 0) s.batch = auto_batch(o, w, s.device, 24.0 * (double)(1ull << 30), true);
        uint64_t bytes = 0;
        cli::check(cpd_batch_bytes(g.n, w.maxdeg, s.batch, &bytes), "batch bytes");
        s.arena = true;
        arena.start(s.device, bytes, o.arena_touch);
    }
    if (o.plan_cache) {
        // workers started together (make_cpds.py:58-60) share one cache:
        // one builds, the others wait for it and load its plan
        int status = 0;
        cli::check(cpd_plan_cache(plan_path.c_str(), g.row_ptr.data(), g.dst.data(), g.w.data(), g.n,
                                  g.m, &po, &s.plan, &status),
                   "plan");
        t.plan_loaded = status == 0;
        std::printf("make_cpd_auto: %s plan %s\n",
                    status == 0 ? "loaded" : status == 1 ? "built and cached" : "built (cache not written)",
                    plan_path.c_str());
    } else {
        cli::check(cpd_plan_create(g.row_ptr.data(), g.dst.data(), g.w.data(), g.n, g.m, &po, &s.plan),
                   "plan");
    }
    t.plan = now() - t0;
    arena.wait();
}

// Uploads the graph, sets the batch (--no-arena with --batch 0: sized here,
// after the contraction, so without its margin) and writes the order file;
// returns the rows per sweep the library settled on.
static uint32_t setup_graph(const Options& o, const Work& w, Session& s, Phases& t) {
    const cpd::io::XYGraph& g = w.g;
    std::vector<uint32_t> order(g.n);
    cli::check(cpd_plan_order(s.plan, order.data()), "order");
    const double t_g0 = now();
    cli::check(cpd_graph_create(s.plan, s.device, &s.dg), "graph upload");
    t.graph = now() - t_g0;
    if (o.reserve_set)
        cli::check(cpd_graph_set_hbm_reserve(s.dg, (uint64_t)o.hbm_reserve), "hbm reserve");
    if (s.batch == 0) s.batch = auto_batch(o, w, s.device, 0.0, false);
    cli::check(cpd_graph_set_batch(s.dg, s.batch), "batch");
    t.batch_alloc = now() - t_g0 - t.graph;
    // the .xy coordinates order each batch's lanes (compact target groups)
    if (g.x.size() == g.n && g.y.size() == g.n)
        cli::check(cpd_graph_set_coords(s.dg, g.x.data(), g.y.data()), "coordinates");
    uint32_t B = 0;
    cli::check(cpd_graph_get_batch(s.dg, &B), "batch");
    cpd::io::write_order(cpd::io::order_path(o.outdir, o.input), w.fp, order);
    t.setup = now() - t_g0;
    return B;
}

// ---- the two writers -------------------------------------------------------

// What a writer did, for report().
struct Totals {
    uint64_t rows = 0, runs = 0;
    // the build calls (sequential: with the export); then what the pipelined
    // build loop stalled on its writers, or the sequential file writes
    double t_build = 0, t_wait = 0;
    // pipelined only.  D2H copies: summed copy time over writer threads,
    // bytes, their wall span (first start to last end); file writes: summed
    // time over threads
    double x_sum = 0, x_span = 0, w_sum = 0;
    uint64_t x_bytes = 0;
};

// Overlapped bucket writer ("overlap D2H of RLE rows with
// the next batch's SSSP, plus parallel bucket-file writes").  Rows are built
// one sweep batch (B rows) per block, in bucket order, alternating between two
// cpd_rows.  While the GPU builds block k+1, a pool of host threads copies
// block k out of HBM in pieces (cpd_rows_export_range: each thread on its own
// stream) and writes each piece straight to its final position in its bucket
// file (BucketFile), so no bucket is ever held whole in host memory.  A
// bucket's .tmp is renamed once its last block is written.  The files are
// byte-identical to the sequential path (--no-pipeline).
// Destinations of the D2H copies: page-locked (cpd_host_alloc), one per
// writer thread, grown on demand.
struct PinnedBuf {
    uint32_t* p = nullptr;
    uint64_t cap = 0;
    uint32_t* get(uint64_t n) {
        if (n > cap) {
            cpd_host_free(p);
            p = nullptr;
            cap = 0;
            void* q = nullptr;
            ok(cpd_host_alloc(std::max<uint64_t>(n, 1) * sizeof(uint32_t), &q), "pinned buffer");
            p = static_cast<uint32_t*>(q);
            cap = n;
        }
        return p;
    }
    ~PinnedBuf() { cpd_host_free(p); }
};

class Pipeline {
public:
    Pipeline(cpd_graph* g, uint32_t B, const Options& o, Totals& tot)
        : g_(g), B_(B), discard_(o.discard), moves_(o.moves), stripes_(o.stripes), tot_(tot) {
        for (int i = 0; i < std::max(1, o.write_threads); ++i) pool_.emplace_back([this] { worker(); });
    }
    ~Pipeline() {
        {
            std::lock_guard<std::mutex> l(mu_);
            stop_ = true;
        }
        cv_.notify_all();
        for (auto& t : pool_) t.join();
        for (cpd_rows* r : rows_)
            if (r) cpd_rows_free(r);
    }

    void run(const std::vector<uint32_t>& targets, const std::vector<uint64_t>& first,
             const std::vector<CpdBucket>& heads, const std::vector<std::string>& paths) {
        using cpd::io::BucketFile;
        using cpd::io::MoveBucketFile;
        const size_t N = targets.size(), nb = heads.size();
        std::vector<std::unique_ptr<BucketFile>> files(nb);
        std::vector<std::unique_ptr<MoveBucketFile>> mfiles(nb);
        std::vector<uint64_t> bruns(nb, 0);  // runs of the bucket's rows scheduled so far
        std::vector<size_t> to_close;        // buckets finished by the block in flight
        uint32_t bits = 4;  // the move tables' width
        if (moves_ && !discard_) ok(cpd_graph_move_bits(g_, &bits), "move bits");
        auto open_bucket = [&](size_t k) {
            if (discard_) return;
            const CpdBucket& h = heads[k];
            if (moves_)
                mfiles[k] = std::make_unique<MoveBucketFile>(
                    paths[k], Work::move_head(h, bits, (uint32_t)(((uint64_t)h.n * bits + 31u) / 32u)),
                    stripes_);
            else files[k] = std::make_unique<BucketFile>(paths[k], h);
        };
        auto close_bucket = [&](size_t k) {
            if (files[k]) files[k]->close(bruns[k]);
            if (mfiles[k]) mfiles[k]->close(bruns[k]);
            files[k].reset();
            mfiles[k].reset();
        };
        for (size_t k = 0; k < nb; ++k)
            if (first[k] == first[k + 1] && !discard_) {  // empty bucket: header (+ one offset)
                open_bucket(k);
                if (files[k]) {
                    const uint64_t zero = 0;
                    files[k]->write_offsets(0, &zero, 1);
                }
                close_bucket(k);
            }
        uint32_t words = 0;  // compact row width
        size_t kb = 0;
        for (size_t b0 = 0, blk = 0; b0 < N; b0 += B_, ++blk) {
            const uint32_t cnt = (uint32_t)std::min<size_t>(B_, N - b0);
            cpd_rows*& r = rows_[blk & 1];
            const double tb = now();
            if (b0 + cnt < N)  // the next block's up-sweep starts beside this block's first moves
                ok(cpd_graph_hint_next(g_, targets.data() + b0 + cnt,
                                       (uint32_t)std::min<size_t>(B_, N - b0 - cnt)),
                   "hint");
            ok(cpd_build_rows(g_, targets.data() + b0, cnt, r, &r), "build");
            tot_.t_build += now() - tb;
            auto offs = std::make_shared<std::vector<uint64_t>>(cnt + 1);
            ok(cpd_rows_export_range(r, 0, cnt, offs->data(), nullptr), "export offsets");
            if (!words) ok(cpd_rows_move_words(r, &words), "move words");
            // block k-1 written (it read the other cpd_rows): close what it finished
            const double tw = now();
            drain();
            tot_.t_wait += now() - tw;
            for (size_t k : to_close) close_bucket(k);
            to_close.clear();
            cpd_rows* rr = r;
            for (size_t i = b0; i < b0 + cnt;) {
                while (first[kb + 1] <= i) ++kb;
                if (!files[kb] && !mfiles[kb]) open_bucket(kb);
                const size_t seg_end = std::min<size_t>(first[kb + 1], b0 + cnt);
                const uint32_t r0 = (uint32_t)(i - b0), r1 = (uint32_t)(seg_end - b0);
                const uint32_t brow0 = (uint32_t)(i - first[kb]);
                const uint64_t base = bruns[kb];
                const bool last = seg_end == first[kb + 1];
                if (moves_)
                    schedule_moves(rr, mfiles[kb].get(), offs, r0, r1, brow0, words);
                else
                    schedule_runs(rr, files[kb].get(), offs, r0, r1, brow0, base, last);
                bruns[kb] += (*offs)[r1] - (*offs)[r0];
                if (last) to_close.push_back(kb);
                i = seg_end;
            }
            tot_.runs += offs->back();
        }
        const double tw = now();
        drain();
        tot_.t_wait += now() - tw;
        for (size_t k : to_close) close_bucket(k);
        tot_.rows = N;
        tot_.x_span = x_last_ > x_first_ ? x_last_ - x_first_ : 0.0;
    }

private:
    // DOSCPD01: bucket-relative offsets (the end offset with the last rows),
    // then the run words in pieces of <= kPieceRuns
    void schedule_runs(cpd_rows* rr, cpd::io::BucketFile* f,
                       const std::shared_ptr<std::vector<uint64_t>>& offs, uint32_t r0, uint32_t r1,
                       uint32_t brow0, uint64_t base, bool last) {
        if (f) submit([=] {
            std::vector<uint64_t> o;
            for (uint32_t u = r0; u < r1 + (last ? 1u : 0u); ++u)
                o.push_back(base + (*offs)[u] - (*offs)[r0]);
            f->write_offsets(brow0, o.data(), (uint32_t)o.size());
        });
        for (uint32_t p0 = r0; p0 < r1;) {
            uint32_t p1 = p0 + 1;
            while (p1 < r1 && (*offs)[p1 + 1] - (*offs)[p0] <= kPieceRuns) ++p1;
            const uint64_t run0 = base + (*offs)[p0] - (*offs)[r0];
            submit([=] {
                thread_local PinnedBuf buf;
                const uint64_t nr = (*offs)[p1] - (*offs)[p0];
                uint32_t* dst = buf.get(nr);
                const double te = now();
                ok(cpd_rows_export_range(rr, p0, p1 - p0, nullptr, dst), "export");
                const double tx = now();
                note_export(te, tx, nr * sizeof(uint32_t));
                if (f) {
                    f->write_runs(run0, dst, nr);
                    note_write(now() - tx);
                }
            });
            p0 = p1;
        }
    }

    // DOSCPD02: the rows' run counts, then the move tables in pieces of
    // <= kPieceRuns words
    void schedule_moves(cpd_rows* rr, cpd::io::MoveBucketFile* f,
                        const std::shared_ptr<std::vector<uint64_t>>& offs, uint32_t r0,
                        uint32_t r1, uint32_t brow0, uint32_t words) {
        if (f) submit([=] {
            std::vector<uint32_t> c(r1 - r0);
            for (uint32_t u = r0; u < r1; ++u) c[u - r0] = (uint32_t)((*offs)[u + 1] - (*offs)[u]);
            f->write_counts(brow0, c.data(), r1 - r0);
        });
        // pieces of <= kPieceRuns words, and at least one per writer thread
        // in a block so the whole pool copies and writes it
        const uint64_t fair = (B_ + pool_.size() - 1) / pool_.size();
        const uint32_t per = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(kPieceRuns / words, fair));
        for (uint32_t p0 = r0; p0 < r1; p0 += per) {
            const uint32_t p1 = std::min(r1, p0 + per);
            submit([=] {
                thread_local PinnedBuf buf;
                const uint64_t nw = (uint64_t)words * (p1 - p0);
                uint32_t* dst = buf.get(nw);
                const double te = now();
                ok(cpd_rows_export_moves(rr, p0, p1 - p0, dst), "export moves");
                const double tx = now();
                note_export(te, tx, nw * sizeof(uint32_t));
                if (f) {
                    f->write_rows(brow0 + (p0 - r0), dst, p1 - p0);
                    note_write(now() - tx);
                }
            });
        }
    }

    void note_export(double t0, double t1, uint64_t bytes) {
        std::lock_guard<std::mutex> l(xmu_);
        tot_.x_sum += t1 - t0;
        tot_.x_bytes += bytes;
        if (x_first_ == 0 || t0 < x_first_) x_first_ = t0;
        x_last_ = std::max(x_last_, t1);
    }
    void note_write(double dt) {
        std::lock_guard<std::mutex> l(xmu_);
        tot_.w_sum += dt;
    }
    std::mutex xmu_;                   // the export and write sums of tot_
    double x_first_ = 0, x_last_ = 0;  // first start / last end of the D2H copies

    static constexpr uint64_t kPieceRuns = 64ull << 20;  // 256 MB of runs / words per copy+write

    void submit(std::function<void()> f) {
        {
            std::lock_guard<std::mutex> l(mu_);
            q_.push_back(std::move(f));
            ++pending_;
        }
        cv_.notify_one();
    }
    void drain() {  // wait for every submitted job; rethrow the first failure
        std::unique_lock<std::mutex> l(mu_);
        done_.wait(l, [this] { return pending_ == 0; });
        if (err_) std::rethrow_exception(err_);
    }
    void worker() {
        for (;;) {
            std::function<void()> f;
            {
                std::unique_lock<std::mutex> l(mu_);
                cv_.wait(l, [this] { return stop_ || !q_.empty(); });
                if (q_.empty()) return;
                f = std::move(q_.front());
                q_.pop_front();
            }
            std::exception_ptr e;
            try {
                f();
            } catch (...) {
                e = std::current_exception();
            }
            std::lock_guard<std::mutex> l(mu_);
            if (e && !err_) err_ = e;
            if (--pending_ == 0) done_.notify_all();
        }
    }

    cpd_graph* g_;
    uint32_t B_;
    bool discard_, moves_;
    uint32_t stripes_;
    Totals& tot_;
    cpd_rows* rows_[2] = {nullptr, nullptr};
    std::vector<std::thread> pool_;
    std::mutex mu_;
    std::condition_variable cv_, done_;
    std::deque<std::function<void()>> q_;
    size_t pending_ = 0;
    bool stop_ = false;
    std::exception_ptr err_;
};

// Every owned row through the Pipeline, in bucket order.
static void write_pipelined(const Options& o, const Work& w, Session& s, uint32_t B, Totals& tot) {
    Pipeline pl(s.dg, B, o, tot);
    const size_t nb = w.owned.size();
    std::vector<uint32_t> targets;
    std::vector<CpdBucket> heads(nb);
    std::vector<uint64_t> first(nb + 1, 0);
    std::vector<std::string> paths(nb);
    for (size_t k = 0; k < nb; ++k) {
        heads[k] = w.head(w.owned[k]);
        paths[k] = w.path(w.owned[k]);
        first[k] = targets.size();
        targets.insert(targets.end(), heads[k].targets.begin(), heads[k].targets.end());
        heads[k].targets.shrink_to_fit();  // every head is held for the whole run
    }
    first[nb] = targets.size();
    pl.run(targets, first, heads, paths);
}

// --no-pipeline: build, then export, then write, a group of buckets at a time.
static void write_sequential(const Options& o, const Work& w, Session& s, uint32_t B, Totals& tot) {
    for (size_t i = 0; i < w.owned.size();) {
        // gather buckets until at least 4 sweeps' worth of rows
        std::vector<CpdBucket> heads;
        std::vector<uint32_t> targets;
        std::vector<size_t> first;
        while (i < w.owned.size() && targets.size() < 4ull * B) {
            heads.push_back(w.head(w.owned[i++]));
            first.push_back(targets.size());
            targets.insert(targets.end(), heads.back().targets.begin(), heads.back().targets.end());
        }
        first.push_back(targets.size());
        const double tb = now();
        cli::check(cpd_build_rows(s.dg, targets.data(), (uint32_t)targets.size(), s.rows, &s.rows), "build");
        uint32_t nr = 0, words = 0, bits = 4;
        uint64_t total = 0;
        cli::check(cpd_rows_count(s.rows, &nr, &total), "rows");
        cli::check(cpd_rows_move_words(s.rows, &words), "move words");
        cli::check(cpd_rows_move_bits(s.rows, &bits), "move bits");
        std::vector<uint64_t> off(nr + 1);
        std::vector<uint32_t> runs(o.moves ? 0 : total), mv(o.moves ? (size_t)nr * words : 0);
        if (o.moves) {
            cli::check(cpd_rows_export_range(s.rows, 0, nr, off.data(), nullptr), "offsets");
            cli::check(cpd_rows_export_moves(s.rows, 0, nr, mv.data()), "export moves");
        } else {
            cli::check(cpd_rows_export(s.rows, off.data(), runs.data()), "export");
        }
        tot.t_build += now() - tb;
        const double ti = now();
        for (size_t k = 0; k < heads.size(); ++k) {
            CpdBucket& b = heads[k];
            const std::string path = w.path(b.bid);
            const uint64_t base = off[first[k]];
            if (o.moves) {
                const uint32_t nb = (uint32_t)b.targets.size();
                std::vector<uint32_t> c(nb);
                for (uint32_t r = 0; r < nb; ++r)
                    c[r] = (uint32_t)(off[first[k] + r + 1] - off[first[k] + r]);
                cpd::io::MoveBucketFile f(path, Work::move_head(b, bits, words), o.stripes);
                f.write_counts(0, c.data(), nb);
                f.write_rows(0, mv.data() + first[k] * (size_t)words, nb);
                f.close(off[first[k + 1]] - base);
                continue;
            }
            for (size_t r = first[k]; r <= first[k + 1]; ++r) b.offsets.push_back(off[r] - base);
            b.runs.assign(runs.begin() + base, runs.begin() + off[first[k + 1]]);
            cpd::io::write_bucket(path, b);
        }
        tot.t_wait += now() - ti;
        tot.rows += nr;
        tot.runs += total;
    }
}

// ---- report ----------------------------------------------------------------

// The line for a person, then one machine-readable line (bench.py's
// full-build leg reads it): rows_s = every owned row built and exported (and
// written, unless --discard); export = the D2H copies (summed over writer
// threads, and their wall span); wait = time the build loop stalled on them
static void report(const Options& o, const Work& w, const cpd_plan_info& info, int device, uint32_t B,
                   const Phases& t, const ArenaStart& arena, const Totals& tot) {
    const double rate = tot.t_build > 0 ? tot.rows / tot.t_build : 0.0;
    std::printf(
        "make_cpd_auto: worker %lld/%lld device %d: %llu rows in %zu buckets, %llu runs "
        "(%.1f per row); read %.3fs plan %.3fs (hierarchy %llu arcs, %u+%u levels) "
        "build %.3fs = %.1f rows/s, %.3f GTEPS; write %.3fs%s; total %.3fs\n",
        o.wid, o.W, device, (unsigned long long)tot.rows, w.owned.size(),
        (unsigned long long)tot.runs, tot.rows ? (double)tot.runs / tot.rows : 0.0, t.read, t.plan,
        (unsigned long long)(info.ch_up_arcs + info.ch_dn_arcs), info.levels_up, info.levels_dn,
        tot.t_build, rate, rate * w.g.m / 1e9, tot.t_wait,
        o.pipeline ? " (not hidden behind the build)" : "", now() - t.start);
    std::printf(
        "make_cpd_auto-json: {\"worker\": %lld, \"maxworker\": %lld, \"rows\": %llu, "
        "\"runs\": %llu, \"batch\": %u, \"discard\": %s, \"read_s\": %.3f, \"plan_s\": %.3f, "
        "\"plan_cached\": %s, \"graph_s\": %.3f, \"batch_alloc_s\": %.3f, \"setup_s\": %.3f, "
        "\"rows_s\": %.3f, \"build_calls_s\": %.3f, \"wait_s\": %.3f, \"free_s\": %.3f, "
        "\"export_bytes\": %llu, \"export_thread_s\": %.3f, \"export_span_s\": %.3f, "
        "\"write_thread_s\": %.3f, \"format\": \"%s\", \"arena_GB\": %.2f, "
        "\"arena_s\": %.3f, \"arena_wait_s\": %.3f, \"total_s\": %.3f}\n",
        o.wid, o.W, (unsigned long long)tot.rows, (unsigned long long)tot.runs, B,
        o.discard ? "true" : "false", t.read, t.plan, t.plan_loaded ? "true" : "false", t.graph,
        t.batch_alloc, t.setup, t.rows, tot.t_build, tot.t_wait, t.free,
        (unsigned long long)tot.x_bytes, tot.x_sum, tot.x_span, tot.w_sum, o.format.c_str(),
        arena.gigabytes(), arena.seconds, arena.waited, now() - t.start);
}

int main(int argc, char** argv) {
    Options o;
    const int refused = parse_options(argc, argv, o);
    if (refused >= 0) return refused;
    ::mkdir(o.outdir.c_str(), 0755);
    Phases t;
    t.start = now();
    try {
        Work w(o);
        t.read = now() - t.start;
        w.list_owned();
        const int full = preflight(o, w);
        if (full >= 0) return full;

        Session s;         // declared first: the arena is released after its thread is joined
        ArenaStart arena;
        make_plan(o, w, s, arena, t);
        if (o.plan_only) {  // warm the cache (host only, no GPU needed)
            std::printf("make_cpd_auto: plan ready in %.3fs\n", t.plan);
            return 0;
        }
        if (s.ndev == 0) {
            std::fprintf(stderr, "make_cpd_auto: no GPU visible (this build has no CPU path)\n");
            return 1;
        }
        cpd_plan_info info{};
        cli::check(cpd_plan_info_get(s.plan, &info), "plan info");
        const uint32_t B = setup_graph(o, w, s, t);

        const double t_rows0 = now();
        Totals tot;
        if (o.pipeline) write_pipelined(o, w, s, B, tot);
        else write_sequential(o, w, s, B, tot);
        t.rows = now() - t_rows0;
        cli::check(s.release(), "arena release");
        t.free = now() - t_rows0 - t.rows;
        report(o, w, info, s.device, B, t, arena, tot);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "make_cpd_auto: %s\n", e.what());
        return 1;
    }
    return 0;
}

