// bin/fifo_auto — drop-in for warthog's resident query server with
// `--alg table-search` (make_fifos.py:20-21, README.md:107-111):
//
//   fifo_auto --input X.xy DIFF --partmethod {div|mod} --partkey K
//             --workerid I --maxworker W --outdir D --alg {table-search|cpd-search}
//             [--partition M] [--device G] [--fifo PATH] [--once]
//             [--index auto|rle|dense] [--read-threads T] [--parse-threads P]
//             [--paths]  (table-search only: also write every walk's nodes)
//             [--search-paths]  (cpd-search only: also write every route's nodes)
//             [--search-loads]  (cpd-search only: also write every edge's load)
//             [--costs [--slice-moves S]]  (table-search only: cost every walk
//                                           under the request's list of diffs)
//             [--loads [--load-slices K --load-slice-moves S]]  (table-search
//                                           only: also write every edge's load)
//             [--timed P [--loads]]  (table-search only: cost, and load, every
//                                     move under the diff of its clock time)
//             [--assign K --capacity C [--vdf A/B^P] [--step msa|line|conj]]  (cpd-search
//                                     only: K iterations of load and re-weight)
//             [--verbose]  (per request on stderr: read+parse / prepare / compute)
//
// Creates its request FIFO, streams the CPD buckets this worker owns onto its
// GPU (as move tables at the graph's packed width when they are smaller
// than the runs, the runs then never held whole in HBM or host memory;
// compact-file pieces read by T threads, default 8), then serves requests on
// /tmp/worker{I}.fifo (process_query.py:86).  A request is what
// process_query.send_remote pipes in (process_query.py:66-79,89):
//     {worker JSON config}\n<query file> <answer fifo> <diff file>\n
// read until the writer closes.  The query file holds "{n}\n" + n "s t" lines
// (process_query.py:93-96).  The answer is ONE line of 10 comma-separated
// values on the answer FIFO (process_query.py:199-208):
//     n_expanded,n_inserted,n_touched,n_updated,n_surplus,plen,finished,
//     t_receive,t_astar,t_search
// For table-search: n_expanded = plen = moves walked, finished = queries that
// reached t, the A*-only fields 0.  For --alg cpd-search (cpd_query_search,
// driven by the request's hscale / fscale / time / itrs / k_moves, the
// library's workspace policy): the five search counters, plen of the paths
// found, finished.  Times in ns for both: t_receive = query file read and
// parse + upload and target sort on the GPU, t_search = the algorithm's
// device time (the walk kernel; the search passes + any table rebuild),
// t_astar = the search passes alone (0 for table-search).  With "debug":
// true in the config, per-query
// results are written to <query file>.res ("s t cost moves finished").
// With --paths (table-search only) every request is answered through
// cpd_query_paths, and when the answer line arrives <query file>.paths holds
// one line per query in file order, "s t finished n v0 v1 ... v(n-1)": the n
// = moves + 1 nodes of the walk from v0 = s (written as .paths.tmp, renamed
// into place).  The answer line is the same with and without it.
// With --search-paths (cpd-search only) every request is answered through
// cpd_query_search_paths and <query file>.paths holds the search paths in
// the same format: the A* tree's chain from s to the incumbent's node, then
// the CPD walk to t; "s t 0 0" (no nodes) for a query without a route.
// With --search-loads (cpd-search only, not with --search-paths) every request
// is answered through cpd_query_search_loads with a demand of 1 per query
// line, not accumulated across requests, and <query file>.loads holds the
// loaded edges of the routes found under the request's diff, in the format
// of --loads below with one column.  The answer line and <query file>.res are
// what they are without it.
// With --costs (table-search only) the request's third field may be a
// comma-separated list of up to 8 diff files, "-" = free flow (e.g.
// "-,a.diff,b.diff"); the walk runs once (cpd_query_costs) and <query
// file>.res gets "s t moves finished cost_0 ... cost_{C-1}" per query in file
// order (written as .res.tmp, renamed into place): C = the number of diffs,
// cost_j the walk's cost under diff j — or, with --slice-moves S, C = 1: move
// h of a walk costed under diff min(h / S, last), a trip replanned every S
// moves.  The answer line keeps its 10 fields and carries no cost.  A
// request's "debug": true writes nothing more with --costs: <query file>.res
// is the costs file.
// With --loads (table-search only) every request is answered through
// cpd_query_loads with a demand of 1 per query line, not accumulated across
// requests, and when the answer line arrives <query file>.loads holds one line
// per edge with any non-zero load, in edge order (the .xy file's):
// "<edge index> <from> <to> <load_0> ... <load_{K-1}>" — K = 1, or with
// --load-slices K --load-slice-moves S the K time slices: move h of a walk
// counts in slice min(h / S, K - 1) (written as .loads.tmp, renamed into
// place).  The answer line and <query file>.res are what they are without it.
// With --timed P (table-search only; 1 <= P <= 2^60, in weight units) every
// request is answered through cpd_query_timed: the request's third field is
// the diff list --costs reads ("-" = free flow, at most 8), diff j the state of
// the network during [j P, (j + 1) P) of clock time, the last open-ended.
// Query line q leaves at the q-th number of <query file>.dep — one unsigned
// integer below 2^63 per query line, in the query file's order — or at 0 when
// that file does not exist; a move is costed under the diff of the time its
// edge is entered and advances the clock by that weight.  <query file>.res
// gets "s t moves finished depart cost" per query in file order (written as
// .res.tmp, renamed into place); "debug": true adds nothing.  With --loads as
// well the call carries CPD_TIMED_LOADS (demand 1 per query line, not
// accumulated across requests) and <query file>.loads holds the loaded edges
// in the format above, one column per diff.  The answer line keeps its fields.
// With --assign K --capacity C (cpd-search only; not with --search-paths,
// --search-loads, --loads or --timed) every request is answered through
// cpd_query_assign: K iterations (1..65535) of cpd_query_search_loads at a
// demand of 1 per query line and cpd_index_weights_from_loads of the mean
// loading, started from the request's diff, every edge at the uniform capacity
// C (1 <= C < 2^32; per-edge capacities are for the ABI) under the delay
// function --vdf A/B^P (default 3/20^4: w' = w0 (1 + A/B (x / C)^P), cpd_api.h
// "The delay function").  The answer line and <query file>.res are the last
// iteration's search.  <query file>.loads holds the summed loadings in the
// format of --loads with one column; <query file>.assign one line per
// iteration, "k finished sptt tstt moves changed" (sptt and tstt in decimal,
// up to 39 digits); <query file>.diff the final weights as "e from to cost"
// lines for the edges that differ from the .xy file's (each written as .tmp
// and renamed into place).  A .diff names an edge by its endpoints, so of
// parallel edges only the first can be re-weighted by it.  Every request
// starts again from its diff: nothing is carried from one request to the next.
// --step line (with --assign; --step msa is the default and changes nothing)
// answers through cpd_query_assign_line instead: the line-search step over the
// flow table (cpd_api.h "The flow step"), at most K iterations — the loop ends
// early after an iteration k >= 2 whose step is 0.  <query file>.assign then
// holds one line per iteration made, "k finished sptt tstt moves changed lambda
// g0 xw0" (lambda in Q16, 0..65536; g0 signed; -g0 / xw0 is the relative gap
// before step k), <query file>.loads the volumes X >> 16 of the final flow in
// the same one-column format, and <query file>.diff the final weights as before.
// --step conj answers through cpd_query_assign_conj (cpd_api.h "The conjugate
// step"): .assign lines are "k finished sptt tstt moves changed lambda gy xw0
// alpha" — the line form's columns with gy where g0 stood, so that minus
// column 8 over column 9 is still the relative gap before step k, then alpha in
// Q16 — and .loads and .diff are as with --step line.
#include <errno.h>
#include <fcntl.h>
#include <signal.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <future>
#include <map>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "cli.hpp"
#include "cpd_io.hpp"

static double now() {
    using namespace std::chrono;
    return duration<double>(steady_clock::now().time_since_epoch()).count();
}

static volatile sig_atomic_t g_stop = 0;
static void on_signal(int) { g_stop = 1; }

// Value of a top-level key in the worker config (json.dumps output), as text.
static std::string json_field(const std::string& js, const std::string& key) {
    std::string pat = "\"" + key + "\"";
    size_t p = js.find(pat);
    if (p == std::string::npos) return "";
    p = js.find(':', p + pat.size());
    if (p == std::string::npos) return "";
    ++p;
    while (p < js.size() && js[p] == ' ') ++p;
    size_t e = p;
    while (e < js.size() && js[e] != ',' && js[e] != '}') ++e;
    std::string v = js.substr(p, e - p);
    while (!v.empty() && v.back() == ' ') v.pop_back();
    return v;
}

static std::string read_all(const std::string& path) {
    int fd = -1;
    while ((fd = ::open(path.c_str(), O_RDONLY)) < 0) {
        if (errno != EINTR || g_stop) return "";
    }
    std::string s;
    char buf[4096];
    for (;;) {
        ssize_t k = ::read(fd, buf, sizeof buf);
        if (k > 0) s.append(buf, (size_t)k);
        else if (k == 0) break;
        else if (errno != EINTR) break;
    }
    ::close(fd);
    return s;
}

// A library call of a request that failed: the request fails (cli::check exits).
static void must(int rc) {
    if (rc != CPD_OK) throw std::runtime_error(cpd_last_error());
}

// A side file of a request, written as <path>.tmp and renamed into place by
// commit(ok: every write succeeded); left any other way, the temporary is
// closed and unlinked.
struct SideFile {
    const std::string path, tmp;
    std::FILE* f;
    explicit SideFile(const std::string& p) : path(p), tmp(p + ".tmp"), f(std::fopen(tmp.c_str(), "w")) {
        if (!f) throw std::runtime_error("cannot write " + tmp + ": " + std::strerror(errno));
    }
    SideFile(const SideFile&) = delete;
    ~SideFile() {
        if (f) std::fclose(f), ::unlink(tmp.c_str());
    }
    void commit(bool ok) {
        ok = std::fclose(f) == 0 && ok;
        f = nullptr;
        place(ok, tmp, path);
    }
    // The tail alone, for a temporary somebody else wrote.
    static void place(bool ok, const std::string& tmp, const std::string& path) {
        if (ok && ::rename(tmp.c_str(), path.c_str()) == 0) return;
        ::unlink(tmp.c_str());
        throw std::runtime_error("cannot write " + path);
    }
};

// <query file>.paths: the walks' nodes, fetched and written in pieces of at
// most ~64M nodes (host memory stays bounded however long the paths are)
static void write_paths(cpd_index* ix, const std::string& qfile, const std::vector<uint32_t>& s,
                        const std::vector<uint32_t>& t, const std::vector<uint64_t>& off) {
    constexpr uint64_t kPiece = 64ull << 20;
    const size_t nq = s.size();
    std::vector<uint8_t> fin(nq);
    must(cpd_query_fetch(ix, nullptr, nullptr, fin.data()));
    SideFile side(qfile + ".paths");
    std::FILE* f = side.f;
    std::vector<uint32_t> nodes;
    std::string out;
    auto put = [&out](uint64_t v, char sep) {
        char d[24];
        int k = 0;
        do d[k++] = (char)('0' + v % 10u); while (v /= 10u);
        while (k) out.push_back(d[--k]);
        out.push_back(sep);
    };
    bool ok = true;
    for (size_t q0 = 0; q0 < nq && ok;) {
        size_t q1 = q0 + 1;
        while (q1 < nq && off[q1 + 1] - off[q0] <= kPiece) ++q1;
        nodes.resize((size_t)(off[q1] - off[q0]));
        must(cpd_query_paths_fetch(ix, (uint32_t)q0, (uint32_t)(q1 - q0), nodes.data()));
        for (size_t q = q0; q < q1; ++q) {
            const uint64_t len = off[q + 1] - off[q];
            put(s[q], ' ');
            put(t[q], ' ');
            put(fin[q] == 1 ? 1u : 0u, ' ');
            put(len, len ? ' ' : '\n');
            const uint32_t* v = nodes.data() + (off[q] - off[q0]);
            for (uint64_t i = 0; i < len; ++i) put(v[i], i + 1 < len ? ' ' : '\n');
            if (out.size() >= (1u << 20)) {
                ok = std::fwrite(out.data(), 1, out.size(), f) == out.size();
                out.clear();
            }
        }
        q0 = q1;
    }
    if (ok && !out.empty()) ok = std::fwrite(out.data(), 1, out.size(), f) == out.size();
    side.commit(ok);
}

// <query file>.res of a --costs request: s t moves finished cost_0 ... per query
static void write_costs(cpd_index* ix, const std::string& qfile, const std::vector<uint32_t>& s,
                        const std::vector<uint32_t>& t, size_t cols) {
    const size_t nq = s.size();
    std::vector<uint64_t> costs(nq * cols);
    std::vector<uint32_t> hops(nq);
    std::vector<uint8_t> fin(nq);
    must(cpd_query_costs_fetch(ix, costs.data(), hops.data(), fin.data()));
    SideFile side(qfile + ".res");
    std::FILE* f = side.f;
    bool ok = true;
    for (size_t q = 0; q < nq && ok; ++q) {
        ok = std::fprintf(f, "%u %u %u %u", s[q], t[q], hops[q], fin[q] == 1 ? 1u : 0u) > 0;
        for (size_t j = 0; j < cols && ok; ++j)
            ok = std::fprintf(f, " %llu", (unsigned long long)costs[q * cols + j]) > 0;
        ok = ok && std::fputc('\n', f) != EOF;
    }
    side.commit(ok);
}

// <query file>.loads: edge from to load_0 ... per edge with any non-zero value
static void write_load_values(const std::string& qfile, const cpd::io::XYGraph& g, size_t slices,
                              const std::vector<uint64_t>& loads) {
    SideFile side(qfile + ".loads");
    std::FILE* f = side.f;
    bool ok = true;
    for (uint32_t a = 0; a < g.n && ok; ++a)
        for (uint32_t e = g.row_ptr[a]; e < g.row_ptr[a + 1] && ok; ++e) {
            bool any = false;
            for (size_t j = 0; j < slices; ++j) any = any || loads[j * g.m + e] != 0;
            if (!any) continue;
            ok = std::fprintf(f, "%u %u %u", e, a, g.dst[e]) > 0;
            for (size_t j = 0; j < slices && ok; ++j)
                ok = std::fprintf(f, " %llu", (unsigned long long)loads[j * g.m + e]) > 0;
            ok = ok && std::fputc('\n', f) != EOF;
        }
    side.commit(ok);
}

// <query file>.loads of a --loads request: the resident table
static void write_loads(cpd_index* ix, const std::string& qfile, const cpd::io::XYGraph& g,
                        size_t slices) {
    std::vector<uint64_t> loads(slices * g.m);
    must(cpd_query_loads_fetch(ix, loads.data()));
    write_load_values(qfile, g, slices, loads);
}

// <query file>.loads of an --assign --step line request: the flow's volumes
static void write_flow(cpd_index* ix, const std::string& qfile, const cpd::io::XYGraph& g) {
    std::vector<uint64_t> x(g.m);
    must(cpd_index_flow_fetch(ix, x.data()));
    for (uint64_t& v : x) v >>= 16;
    write_load_values(qfile, g, 1, x);
}

// a 128-bit unsigned value in decimal
static std::string dec128(uint64_t lo, uint64_t hi) {
    unsigned __int128 v = ((unsigned __int128)hi << 64) | lo;
    std::string d;
    do d.insert(d.begin(), (char)('0' + (int)(v % 10u))); while (v /= 10u);
    return d;
}

// a 128-bit signed value (two's complement halves) in decimal
static std::string dec128_signed(uint64_t lo, uint64_t hi) {
    if (!(hi >> 63)) return dec128(lo, hi);
    const unsigned __int128 v = ~(((unsigned __int128)hi << 64) | lo) + 1u;
    return "-" + dec128((uint64_t)v, (uint64_t)(v >> 64));
}

// <query file>.assign and <query file>.diff of an --assign request: one line
// of text per iteration, then the final weights
static void write_assign(cpd_index* ix, const std::string& qfile, const cpd::io::XYGraph& g,
                         const std::vector<std::string>& lines) {
    {
        SideFile side(qfile + ".assign");
        bool ok = true;
        for (size_t k = 0; k < lines.size() && ok; ++k)
            ok = std::fprintf(side.f, "%zu %s\n", k + 1, lines[k].c_str()) > 0;
        side.commit(ok);
    }
    std::vector<uint32_t> w(g.m);
    must(cpd_index_get_weights(ix, w.data()));
    const std::string path = qfile + ".diff", tmp = path + ".tmp";
    cpd::io::write_diff(tmp, g, w);  // the library's writer; a throw leaves its temporary as it is
    SideFile::place(true, tmp, path);
}

// What follows the common fields on an .assign line: the rule's step and gap terms.
static std::string assign_tail(const cpd_assign_iter&) { return ""; }
static std::string assign_tail(const cpd_assign_line_iter& r) {
    return " " + std::to_string(r.lambda_q16) + " " + dec128_signed(r.g0_lo, r.g0_hi) + " " +
           dec128(r.xw0_lo, r.xw0_hi);
}
static std::string assign_tail(const cpd_assign_conj_iter& r) {
    return " " + std::to_string(r.lambda_q16) + " " + dec128_signed(r.gy_lo, r.gy_hi) + " " +
           dec128(r.xw0_lo, r.xw0_hi) + " " + std::to_string(r.alpha_q16);
}

// cpd_query_assign in the other two loops' shape: it makes every record.
static int assign_msa(cpd_index* ix, const cpd_search_opts* opts, uint64_t prefix_bytes,
                      const uint32_t* demand, const uint32_t* capacity, const cpd_vdf* f,
                      uint32_t iters, cpd_assign_iter* out, uint32_t* done) {
    *done = iters;
    return cpd_query_assign(ix, opts, prefix_bytes, demand, capacity, f, iters, out);
}

// An --assign request through one of the three loops (demand 1 per query):
// the text of one .assign line per record made; returns their summed search_ms.
template <class Rec>
static double run_assign(int (*loop)(cpd_index*, const cpd_search_opts*, uint64_t, const uint32_t*,
                                     const uint32_t*, const cpd_vdf*, uint32_t, Rec*, uint32_t*),
                         cpd_index* ix, const cpd_search_opts& so, const std::vector<uint32_t>& cap,
                         const cpd_vdf& vdf, uint32_t iters, std::vector<std::string>& lines) {
    std::vector<Rec> it(iters);
    uint32_t made = 0;
    must(loop(ix, &so, 0, nullptr, cap.data(), &vdf, iters, it.data(), &made));
    double search_ms = 0.0;
    for (uint32_t k = 0; k < made; ++k) {
        const Rec& r = it[k];
        lines.push_back(std::to_string(r.finished) + " " + dec128(r.sptt_lo, r.sptt_hi) + " " +
                        dec128(r.tstt_lo, r.tstt_hi) + " " + std::to_string(r.moves) + " " +
                        std::to_string(r.changed) + assign_tail(r));
        search_ms += r.search_ms;
    }
    return search_ms;
}

// <query file>.dep of a --timed request: one unsigned integer per query line;
// no such file: every query leaves at 0 (dep stays empty)
static void read_departures(const std::string& qfile, size_t nq, std::vector<uint64_t>& dep) {
    dep.clear();
    const std::string path = qfile + ".dep";
    std::FILE* f = std::fopen(path.c_str(), "r");
    if (!f) {
        if (errno == ENOENT) return;
        throw std::runtime_error("cannot read " + path + ": " + std::strerror(errno));
    }
    std::string text;
    char buf[65536];
    for (size_t k; (k = std::fread(buf, 1, sizeof buf, f)) > 0;) text.append(buf, k);
    std::fclose(f);
    dep.reserve(nq);
    size_t line = 1;
    for (size_t p = 0; p < text.size(); ++line) {
        size_t e = text.find('\n', p);
        if (e == std::string::npos) e = text.size();
        size_t a = p, b = e;
        while (a < b && (text[a] == ' ' || text[a] == '\t')) ++a;
        while (b > a && (text[b - 1] == ' ' || text[b - 1] == '\t' || text[b - 1] == '\r')) --b;
        uint64_t v = 0;
        bool ok = a < b;
        for (size_t i = a; i < b && ok; ++i) {
            const unsigned d = (unsigned)(text[i] - '0');
            ok = d <= 9u && v <= (0xFFFFFFFFFFFFFFFFull - d) / 10u;
            v = v * 10u + d;
        }
        if (!ok)
            throw std::runtime_error(path + ": line " + std::to_string(line) +
                                     " is not an unsigned integer");
        dep.push_back(v);
        p = e + 1;
    }
    if (dep.size() != nq)
        throw std::runtime_error(path + ": " + std::to_string(dep.size()) + " departures for " +
                                 std::to_string(nq) + " queries");
}

// <query file>.res of a --timed request: s t moves finished depart cost per query
static void write_timed(cpd_index* ix, const std::string& qfile, const std::vector<uint32_t>& s,
                        const std::vector<uint32_t>& t, const std::vector<uint64_t>& dep) {
    const size_t nq = s.size();
    std::vector<uint64_t> cost(nq);
    std::vector<uint32_t> hops(nq);
    std::vector<uint8_t> fin(nq);
    must(cpd_query_timed_fetch(ix, cost.data(), hops.data(), fin.data()));
    SideFile side(qfile + ".res");
    bool ok = true;
    for (size_t q = 0; q < nq && ok; ++q)
        ok = std::fprintf(side.f, "%u %u %u %u %llu %llu\n", s[q], t[q], hops[q],
                          fin[q] == 1 ? 1u : 0u, (unsigned long long)(dep.empty() ? 0 : dep[q]),
                          (unsigned long long)cost[q]) > 0;
    side.commit(ok);
}

static bool write_answer(const std::string& path, const std::string& line) {
    // process_query.send_remote mkfifo's the answer before writing the request
    // (process_query.py:72-73); tolerate a late mkfifo for up to 10 s
    for (int i = 0; i < 1000; ++i) {
        struct stat st;
        if (::stat(path.c_str(), &st) == 0) break;
        std::this_thread::sleep_for(std::chrono::milliseconds(10));
    }
    int fd = ::open(path.c_str(), O_WRONLY);
    if (fd < 0) return false;
    std::string out = line + "\n";
    const char* p = out.data();
    size_t left = out.size();
    while (left) {
        ssize_t k = ::write(fd, p, left);
        if (k < 0) {
            if (errno == EINTR) continue;
            ::close(fd);
            return false;
        }
        p += k;
        left -= (size_t)k;
    }
    ::close(fd);
    return true;
}

// ---- options ---------------------------------------------------------------

// How every request of this server is answered: the call behind it, those of
// --alg table-search first, then those of --alg cpd-search.
enum class Mode { Run, Paths, Costs, Loads, Timed, Search, SearchPaths, SearchLoads, Assign };
enum class Step { Msa, Line, Conj };  // the --assign loop's step rule

// --alg cpd-search: the answer line carries the search counters
static bool is_search(Mode m) { return m >= Mode::Search; }
// the diff field is a list of weight sets, and <query file>.res the mode's own
// file ("debug": true adds nothing)
static bool lists_diffs(Mode m) { return m == Mode::Costs || m == Mode::Timed; }

// Everything read from argv; the numbers are in the ranges parse_options checks.
struct Options {
    std::vector<std::string> inputs;  // X.xy [DIFF]
    std::string method, outdir, fifo, index, device;  // device "": worker id modulo the devices
    long long key = -1, wid = -1, W = -1;
    int mcode = 0;
    Mode mode = Mode::Run;
    bool timed_loads = false;  // --timed with --loads
    Step step = Step::Msa;
    long long slice_moves = 0, load_slices = 1, load_slice_moves = 0, period = 0;
    long long assign_iters = 0, assign_cap = 0;
    cpd_vdf vdf{3, 20, 4, 1};
    int read_threads = 8, parse_threads = 16;
    bool once = false, verbose = false;
    const std::string& xy() const { return inputs[0]; }
};

static const char kUsage[] =
    "usage: fifo_auto --input X.xy [DIFF] --partmethod {div|mod} --partkey K --workerid I --maxworker W --outdir D --alg table-search|cpd-search\n"
    "       [--paths]  table-search only: answer through cpd_query_paths and write every\n"
    "                  walk's nodes to <query file>.paths, one line per query:\n"
    "                  s t finished n v0 ... v(n-1)\n"
    "       [--search-paths]  cpd-search only: answer through cpd_query_search_paths and\n"
    "                  write every route's nodes to <query file>.paths, same format\n"
    "       [--search-loads]  cpd-search only: answer through cpd_query_search_loads (demand 1\n"
    "                  per query) and write every loaded edge of the routes found to\n"
    "                  <query file>.loads: edge from to load\n"
    "       [--costs [--slice-moves S]]  table-search only: the request's diff field may list\n"
    "                  up to 8 diffs (\"-,a.diff,b.diff\"); one walk costs every query under each\n"
    "                  (cpd_query_costs) and <query file>.res gets, per query:\n"
    "                  s t moves finished cost_0 ... cost_{C-1}\n"
    "                  (with --slice-moves S one cost: move h under diff min(h / S, last));\n"
    "                  \"debug\": true in a request adds nothing: .res is the costs file\n"
    "       [--loads [--load-slices K --load-slice-moves S]]  table-search only: answer through\n"
    "                  cpd_query_loads (demand 1 per query) and write every loaded edge to\n"
    "                  <query file>.loads: edge from to load_0 ... load_{K-1}\n"
    "                  (K slices: move h counts in slice min(h / S, K - 1))\n"
    "       [--timed P [--loads]]  table-search only: answer through cpd_query_timed; the\n"
    "                  request's diff field lists up to 8 diffs, diff j the network during clock\n"
    "                  time [j P, (j + 1) P); departures from <query file>.dep (one per query\n"
    "                  line; absent: 0); <query file>.res gets, per query:\n"
    "                  s t moves finished depart cost\n"
    "                  (with --loads <query file>.loads has one column per diff)\n"
    "       [--assign K --capacity C [--vdf A/B^P]]  cpd-search only: answer through\n"
    "                  cpd_query_assign (K iterations, demand 1 per query, every edge at capacity C,\n"
    "                  delay w0 (1 + A/B (x/C)^P), default 3/20^4); writes <query file>.loads,\n"
    "                  .assign (k finished sptt tstt moves changed) and .diff (the final weights)\n"
    "       [--step msa|line|conj]  with --assign: msa (default) as above; line answers through\n"
    "                  cpd_query_assign_line (the line-search step): .assign lines end in\n"
    "                  lambda g0 xw0, .loads holds the final flow's volumes; conj answers through\n"
    "                  cpd_query_assign_conj (the conjugate step): .assign lines end in lambda gy xw0 alpha\n";

// How every check below refuses: its text on stderr, exit status 2.
static int refuse(const char* text) {
    std::fputs(text, stderr);
    return 2;
}

// Fills `o` from argv.  The checks run in this order, before anything is read
// or made; returns the exit status of the first that fails, or -1 to go on.
static int parse_options(int argc, char** argv, Options& o) {
    cli::Args a(argc, argv);
    o.inputs = a.list("input");
    o.method = a.str_any({"partmethod", "partition"});
    o.key = a.num("partkey", -1), o.wid = a.num("workerid", -1), o.W = a.num("maxworker", -1);
    const std::string alg = a.str("alg", "table-search");
    if (o.inputs.empty() || o.method.empty() || o.key <= 0 || o.wid < 0 || o.W <= 0 || o.wid >= o.W)
        return refuse(kUsage);
    // table-search (make_fifos.py:20) or the CPD-heuristic search
    // (cpd_query_search; args.py:29-57)
    const bool search = alg == "cpd-search" || alg == "cpd_search";
    if (alg != "table-search" && !search) {
        std::fprintf(stderr, "fifo_auto: --alg must be table-search or cpd-search (got '%s')\n",
                     alg.c_str());
        return 2;
    }
    const bool paths = a.has("paths");
    if (paths && search)
        return refuse("fifo_auto: --paths needs --alg table-search (the paths of a "
                      "cpd-search are extracted with --search-paths)\n");
    const bool search_paths = a.has("search-paths");
    if (search_paths && !search)
        return refuse("fifo_auto: --search-paths needs --alg cpd-search (the walks of a "
                      "table-search are extracted with --paths)\n");
    const bool costs = a.has("costs");
    if (costs && (search || paths))
        return refuse("fifo_auto: --costs needs --alg table-search without --paths (a "
                      "cpd-search's route depends on the weights; --paths answers through "
                      "cpd_query_paths)\n");
    o.slice_moves = a.num("slice-moves", 0);
    if ((o.slice_moves && !costs) || o.slice_moves < 0 || o.slice_moves > 0xFFFFFFFFll)
        return refuse("fifo_auto: --slice-moves S needs --costs and 0 <= S < 2^32\n");
    const bool loads = a.has("loads");
    if (loads && (search || paths || costs))
        return refuse("fifo_auto: --loads needs --alg table-search without --paths or "
                      "--costs (a cpd-search's route is not the walk's: --search-loads loads "
                      "it; --paths and --costs "
                      "answer through cpd_query_paths and cpd_query_costs)\n");
    const bool slices = a.has("load-slices") || a.has("load-slice-moves");
    const bool timed = a.has("timed");
    if (timed && (search || paths || costs || slices))
        return refuse("fifo_auto: --timed needs --alg table-search without --paths, --costs, "
                      "--load-slices or --load-slice-moves (a cpd-search's route is not the "
                      "walk's; --paths and --costs answer through cpd_query_paths and "
                      "cpd_query_costs; a timed walk's load planes are its diffs)\n");
    o.period = a.num("timed", 0);
    if (timed && (o.period < 1 || o.period > (1ll << 60)))
        return refuse("fifo_auto: --timed P needs 1 <= P <= 2^60\n");
    const bool search_loads = a.has("search-loads");
    if (search_loads && (!search || search_paths || slices))
        return refuse("fifo_auto: --search-loads needs --alg cpd-search without --search-paths, "
                      "--load-slices or --load-slice-moves (the walks of a table-search are "
                      "loaded with --loads; --search-paths answers through "
                      "cpd_query_search_paths; a search loads one plane)\n");
    o.load_slices = a.num("load-slices", 1), o.load_slice_moves = a.num("load-slice-moves", 0);
    if ((slices && !loads) || o.load_slices < 1 || o.load_slices > (long long)CPD_MAX_LOAD_SLICES ||
        o.load_slice_moves < 0 || o.load_slice_moves > 0xFFFFFFFFll ||
        (o.load_slices == 1) != (o.load_slice_moves == 0)) {
        std::fprintf(stderr, "fifo_auto: --load-slices K --load-slice-moves S need --loads, 2 <= K "
                             "<= %u and 0 < S < 2^32 (both or neither)\n", CPD_MAX_LOAD_SLICES);
        return 2;
    }
    const bool assign = a.has("assign");
    if (assign && (!search || search_paths || search_loads || loads || timed))
        return refuse("fifo_auto: --assign needs --alg cpd-search without --search-paths, "
                      "--search-loads, --loads or --timed (the loop answers through "
                      "cpd_query_assign and writes the loads itself)\n");
    o.assign_iters = a.num("assign", 0), o.assign_cap = a.num("capacity", 0);
    unsigned an = 0, ad = 0, pw = 0;
    char tail = 0;
    const bool vdf_ok =
        std::sscanf(a.str("vdf", "3/20^4").c_str(), "%u/%u^%u%c", &an, &ad, &pw, &tail) == 3 &&
        an <= 65535u && ad >= 1u && ad <= 65535u && pw >= 1u && pw <= 4u;
    if ((a.has("vdf") || a.has("capacity")) && !assign)
        return refuse("fifo_auto: --capacity and --vdf need --assign\n");
    if (assign && (!vdf_ok || o.assign_iters < 1 || o.assign_iters > 65535 || o.assign_cap < 1 ||
                   o.assign_cap > 0xFFFFFFFFll))
        return refuse("fifo_auto: --assign K --capacity C [--vdf A/B^P] need 1 <= K <= "
                      "65535, 1 <= C < 2^32, A <= 65535, 1 <= B <= 65535 and 1 <= P <= 4\n");
    o.vdf = cpd_vdf{an, ad, pw, 1};
    const std::string step = a.str("step", "msa");
    if ((a.has("step") && !assign) || (step != "msa" && step != "line" && step != "conj"))
        return refuse("fifo_auto: --step msa|line|conj needs --assign\n");
    o.step = step == "line" ? Step::Line : step == "conj" ? Step::Conj : Step::Msa;
    o.mcode = cli::method_code(o.method);
    // what passed the checks names one way of answering
    o.mode = assign         ? Mode::Assign
             : search_paths ? Mode::SearchPaths
             : search_loads ? Mode::SearchLoads
             : search       ? Mode::Search
             : costs        ? Mode::Costs
             : timed        ? Mode::Timed
             : loads        ? Mode::Loads
             : paths        ? Mode::Paths
                            : Mode::Run;
    o.timed_loads = timed && loads;
    o.outdir = a.str("outdir", ".");
    o.fifo = a.str("fifo", "/tmp/worker" + std::to_string(o.wid) + ".fifo");
    o.index = a.str("index", "auto");
    o.device = a.str("device");
    o.read_threads = (int)a.num("read-threads", 8);
    // threads parsing a request's query file (a 1M-query file is ~14 MB)
    o.parse_threads = (int)a.num("parse-threads", 16);
    o.once = a.has("once");
    o.verbose = a.has("verbose");
    return -1;
}

// ---- start-up load ---------------------------------------------------------

// The request FIFO exists before the (possibly long) index load: a request
// sent meanwhile blocks in its writer's open() until the serve loop reads it,
// instead of `cat <<CONF > fifo` creating a regular file there.  A non-FIFO
// left at the path (such a file from an earlier run) is replaced.
static bool make_fifo(const std::string& fifo) {
    struct stat st;
    if (::lstat(fifo.c_str(), &st) == 0 && !S_ISFIFO(st.st_mode)) ::unlink(fifo.c_str());
    if (::mkfifo(fifo.c_str(), 0666) != 0 && errno != EEXIST) {
        std::fprintf(stderr, "fifo_auto: mkfifo %s: %s\n", fifo.c_str(), std::strerror(errno));
        return false;
    }
    if (::lstat(fifo.c_str(), &st) == 0 && S_ISFIFO(st.st_mode)) return true;
    std::fprintf(stderr, "fifo_auto: %s is not a FIFO\n", fifo.c_str());
    return false;
}

// What the load leaves for the serve loop; unload() frees it.
struct Loaded {
    cpd_plan* plan = nullptr;
    cpd_graph* dg = nullptr;
    cpd_index* ix = nullptr;
    cpd::io::XYGraph g;
    std::map<std::string, std::vector<uint32_t>> diff_cache;
    int device = -1;
    bool arena = false;
};

static void unload(Loaded& L) {
    cpd_index_free(L.ix);
    cpd_graph_free(L.dg);
    cpd_plan_free(L.plan);
    if (L.arena) cpd_device_arena_release(L.device);
}

// The weights a diff file gives the graph's edges, read once per name.
static const std::vector<uint32_t>& diff_weights(Loaded& L, const std::string& name) {
    auto it = L.diff_cache.find(name);
    if (it == L.diff_cache.end()) it = L.diff_cache.emplace(name, cpd::io::read_diff(name, L.g)).first;
    return it->second;
}

// This worker's buckets, headers only (targets, run counts or offsets), in
// bucket order: formats[k] says whether heads[k] or mheads[k] is filled.
struct Heads {
    uint32_t n0 = 0;  // the node count, from the order file
    std::vector<std::string> paths;
    std::vector<int> formats;  // 1: run words; 2: compact move tables
    std::vector<cpd::io::CpdBucket> heads;
    std::vector<cpd::io::MoveBucket> mheads;
    std::vector<uint32_t> targets;
    uint64_t total_runs = 0, compact_bytes = 0;
    uint32_t move_bits = 0;  // the compact rows' width (0: some bucket holds run words)
    bool all_compact = true;
};

// DOSCPD02/03 (compact move tables, what make_cpd_auto writes by default) or
// DOSCPD01 (run words).  The node count comes from the order file
// make_cpd_auto wrote beside them; the graph's fingerprint is checked once the
// .xy is read.
static Heads read_heads(const Options& o) {
    Heads h;
    h.n0 = cpd::io::read_order_n(cpd::io::order_path(o.outdir, o.xy()));
    uint32_t nb = 0;
    cli::check(cpd_partition_nbuckets(h.n0, o.mcode, (uint32_t)o.key, &nb), "buckets");
    for (uint32_t b = 0; b < nb; ++b) {
        if (b % (uint32_t)o.W != (uint32_t)o.wid) continue;
        h.paths.push_back(cpd::io::bucket_path(o.outdir, o.xy(), o.method, (uint32_t)o.key, b));
        h.formats.push_back(cpd::io::bucket_format(h.paths.back()));
        if (h.formats.back() == 1) {
            h.heads.push_back(cpd::io::read_bucket_head(h.paths.back()));
            h.mheads.emplace_back();
            const auto& bk = h.heads.back();
            h.targets.insert(h.targets.end(), bk.targets.begin(), bk.targets.end());
            h.total_runs += bk.offsets.back();
            h.all_compact = false;
        } else {
            h.mheads.push_back(cpd::io::read_move_bucket_head(h.paths.back()));
            h.heads.emplace_back();
            const auto& bk = h.mheads.back();
            if (bk.n != h.n0) throw std::runtime_error("bucket " + std::to_string(b) + " has another node count");
            h.targets.insert(h.targets.end(), bk.targets.begin(), bk.targets.end());
            h.total_runs += bk.total_runs;
            h.compact_bytes += 4ull * bk.words * bk.targets.size();
            h.move_bits = bk.bits;
        }
    }
    return h;
}

// The device side, started on a thread beside the host reads (VERDICT r04
// item 7): the first HIP call and, for compact buckets, the dense index's HBM
// committed as an arena (nrows x n padded to 2048 columns x bits / 8 bytes:
// committing fresh HBM costs about a second per 30 GB) that
// cpd_index_create_empty then carves.  Joined by the caller, or on the way
// out; `o` and `h` outlive it.
struct DeviceStart {
    int ndev = 0, rc = CPD_OK, device = -1;
    bool arena = false;
    double seconds = 0.0;
    std::string err;
    std::thread thr;
    DeviceStart(const Options& o, const Heads& h) : thr([this, &o, &h] { run(o, h); }) {}
    ~DeviceStart() {
        if (thr.joinable()) thr.join();
    }
    void run(const Options& o, const Heads& h) {
        const double td = now();
        rc = cpd_device_count(&ndev);
        if (rc == CPD_OK && ndev > 0) {
            device = (int)(o.device.empty() ? o.wid % ndev : std::atoll(o.device.c_str()));
            if (h.all_compact && !h.targets.empty() && h.move_bits) {
                const uint64_t npad = (h.n0 + 2047ull) / 2048ull * 2048ull;
                const uint64_t bytes = (uint64_t)h.targets.size() * (npad * h.move_bits / 32ull) * 4ull;
                // only for an index that will be dense (--index rle keeps
                // runs; auto takes tables when the runs weigh more — the
                // index's own test): an unused arena would hold HBM the
                // search workspace is sized from
                const bool dense = o.index == "dense" || (o.index != "rle" && 4ull * h.total_runs > bytes);
                if (dense) arena = cpd_device_arena(device, bytes + (1ull << 20), 0) == CPD_OK;
            }
        }
        if (rc != CPD_OK) err = cpd_last_error();
        seconds = now() - td;
    }
};

// The graph, the plan, the start diff's weights, and the checks that the index
// on disk is this graph's: the stored column order against this build's, and
// every bucket's fingerprint, key and method.
static void load_graph(const Options& o, const Heads& h, Loaded& L) {
    const cpd::io::XYGraph& g = L.g = cpd::io::read_xy(o.xy());
    const uint64_t fp = cpd::io::graph_fingerprint(g.n, g.row_ptr.data(), g.dst.data(), g.w.data());
    if (o.inputs.size() > 1) diff_weights(L, o.inputs[1]);
    cpd_plan_opts po{};
    po.no_hierarchy = 1;  // queries need the CSR + column order only
    cli::check(cpd_plan_create(g.row_ptr.data(), g.dst.data(), g.w.data(), g.n, g.m, &po, &L.plan),
               "plan");
    std::vector<uint32_t> order(g.n);
    cli::check(cpd_plan_order(L.plan, order.data()), "order");
    if (cpd::io::read_order(cpd::io::order_path(o.outdir, o.xy()), fp) != order)
        throw std::runtime_error("stored column order differs from this build's");
    for (size_t k = 0; k < h.paths.size(); ++k) {
        const bool rle = h.formats[k] == 1;
        const uint64_t bfp = rle ? h.heads[k].fingerprint : h.mheads[k].fingerprint;
        const uint32_t bkey = rle ? h.heads[k].key : h.mheads[k].key;
        const uint32_t bmethod = rle ? h.heads[k].method : h.mheads[k].method;
        if (bfp != fp || bkey != (uint32_t)o.key || bmethod != (uint32_t)o.mcode)
            throw std::runtime_error(h.paths[k] + " was built for another graph/partition");
    }
}

// The rows are streamed in pieces of <= kPiece words (a longer row alone): a
// dense index never holds the worker's runs in HBM or RAM.
constexpr uint64_t kPiece = 64ull << 20;  // 256 MB

// The two page-locked buffers the compact pieces are read into.
struct PinnedPair {
    uint32_t* p[2] = {nullptr, nullptr};
    uint64_t bytes = 0;
    PinnedPair() = default;
    PinnedPair(const PinnedPair&) = delete;
    ~PinnedPair() {
        for (auto q : p) cpd_host_free(q);
    }
};

// One compact bucket: its pieces read into the two buffers by a reader
// thread while the previous piece is appended (uploaded).
static void stream_compact(cpd_index* ix, const std::string& path, const cpd::io::MoveBucket& mh,
                           int read_threads, PinnedPair& pin) {
    const uint32_t nr = (uint32_t)mh.targets.size();
    if (!nr) return;
    const uint32_t per = (uint32_t)std::min<uint64_t>(nr, std::max<uint64_t>(1, kPiece / mh.words));
    if (4ull * mh.words * per > pin.bytes) {  // grown for this bucket's pieces
        for (auto& p : pin.p) {
            cpd_host_free(p);
            void* q = nullptr;
            cli::check(cpd_host_alloc(4ull * mh.words * per, &q), "pinned buffer");
            p = static_cast<uint32_t*>(q);
        }
        pin.bytes = 4ull * mh.words * per;
    }
    auto read = [&](uint32_t r0, int slot) {
        cpd::io::read_move_bucket_rows(path, mh, r0, std::min(per, nr - r0), pin.p[slot], read_threads);
    };
    std::future<void> rd = std::async(std::launch::async, read, 0u, 0);
    for (uint32_t r0 = 0, i = 0; r0 < nr; r0 += per, ++i) {
        rd.get();  // piece i is in pin.p[i & 1] (a read error is rethrown here)
        if (r0 + per < nr) rd = std::async(std::launch::async, read, r0 + per, (int)((i + 1) & 1u));
        const int rc = cpd_index_append_moves(ix, std::min(per, nr - r0), mh.bits, pin.p[i & 1u]);
        if (rc != CPD_OK) {
            if (rd.valid()) rd.wait();
            cli::check(rc, "index rows");
        }
    }
}

// One bucket of run words, piece by piece through `buf` (offsets through `rel`).
static void stream_runs(cpd_index* ix, const std::string& path, const cpd::io::CpdBucket& head,
                        std::vector<uint32_t>& buf, std::vector<uint64_t>& rel) {
    const auto& off = head.offsets;
    const uint32_t nr = (uint32_t)head.targets.size();
    for (uint32_t r0 = 0; r0 < nr;) {
        uint32_t r1 = r0 + 1;
        while (r1 < nr && off[r1 + 1] - off[r0] <= kPiece) ++r1;
        buf.resize(off[r1] - off[r0]);
        cpd::io::read_bucket_runs(path, head, off[r0], buf.size(), buf.data());
        rel.resize(r1 - r0 + 1);
        for (uint32_t i = r0; i <= r1; ++i) rel[i - r0] = off[i] - off[r0];
        cli::check(cpd_index_append_rows(ix, r1 - r0, rel.data(), buf.data()), "index rows");
        r0 = r1;
    }
}

// Streams the CPD buckets this worker owns onto its GPU and says so: the
// machine-readable line (bench.py's full-build leg reads it), then the
// "listening" line a driver waits for.
static Loaded load(const Options& o) {
    Loaded L;
    const double t0 = now();
    const Heads h = read_heads(o);
    DeviceStart dev(o, h);
    load_graph(o, h, L);
    const double t_graph0 = now();
    dev.thr.join();
    const double t_devwait = now() - t_graph0;
    if (dev.rc != CPD_OK) throw std::runtime_error("device: " + dev.err);
    if (dev.ndev == 0) throw std::runtime_error("no GPU visible (this build has no CPU path)");
    L.device = dev.device;
    L.arena = dev.arena;
    cli::check(cpd_graph_create(L.plan, L.device, &L.dg), "graph upload");
    const int imode = o.index == "rle" ? CPD_INDEX_RLE : o.index == "dense" ? CPD_INDEX_DENSE : CPD_INDEX_AUTO;
    cli::check(cpd_index_create_empty(L.dg, h.targets.data(), (uint32_t)h.targets.size(), imode,
                                      h.total_runs, &L.ix),
               "index");
    const double t_rows0 = now();
    {
        std::vector<uint32_t> buf;
        std::vector<uint64_t> rel;
        PinnedPair pin;
        for (size_t k = 0; k < h.paths.size(); ++k) {
            if (h.formats[k] == 2) stream_compact(L.ix, h.paths[k], h.mheads[k], o.read_threads, pin);
            else stream_runs(L.ix, h.paths[k], h.heads[k], buf, rel);
        }
    }
    const double t_rows = now() - t_rows0;
    int mode = 0;
    cli::check(cpd_index_get_mode(L.ix, &mode), "index mode");
    const char* index = mode == CPD_INDEX_DENSE ? "dense" : "rle";
    std::printf("fifo_auto-json: {\"worker\": %lld, \"rows\": %zu, \"runs\": %llu, "
                "\"index\": \"%s\", \"compact_bytes\": %llu, \"read_plan_s\": %.3f, "
                "\"device_s\": %.3f, \"device_wait_s\": %.3f, \"arena\": %s, "
                "\"graph_s\": %.3f, \"rows_s\": %.3f, \"ready_s\": %.3f}\n",
                o.wid, h.targets.size(), (unsigned long long)h.total_runs, index,
                (unsigned long long)h.compact_bytes, t_graph0 - t0, dev.seconds, t_devwait,
                L.arena ? "true" : "false", t_rows0 - t_graph0, t_rows, now() - t0);
    std::printf("fifo_auto: worker %lld: %zu rows, %llu runs (%s index) on device %d, ready in "
                "%.3fs; listening on %s\n",
                o.wid, h.targets.size(), (unsigned long long)h.total_runs, index, L.device,
                now() - t0, o.fifo.c_str());
    std::fflush(stdout);
    return L;
}

// ---- a request -------------------------------------------------------------

// One message on the request FIFO, taken apart.
struct Request {
    std::string qfile, answer, diff;  // diff: "-" when the third field is absent
    int k_moves = -1;
    bool debug = false;
    cpd_search_opts so{};
};

// False (and a line on stderr) for a message without a query file and an
// answer FIFO.  Every key of the config is read once.
static bool parse_request(const std::string& msg, Request& r) {
    const size_t nl = msg.find('\n');
    const std::string conf = msg.substr(0, nl);
    const std::string rest = nl == std::string::npos ? "" : msg.substr(nl + 1);
    char qfile[4096] = {0}, answer[4096] = {0}, dname[4096] = {0};
    const int got = std::sscanf(rest.c_str(), "%4095s %4095s %4095s", qfile, answer, dname);
    if (got < 2) {
        std::fprintf(stderr, "fifo_auto: malformed request: %s\n", msg.c_str());
        return false;
    }
    r.qfile = qfile, r.answer = answer, r.diff = got >= 3 ? dname : "-";
    const std::string km = json_field(conf, "k_moves"), hscale = json_field(conf, "hscale"),
                      fscale = json_field(conf, "fscale"), itrs = json_field(conf, "itrs"),
                      time = json_field(conf, "time");
    r.k_moves = km.empty() ? -1 : std::atoi(km.c_str());
    r.debug = json_field(conf, "debug") == "true";
    // cpd-search knobs (process_query.py:149-160): hscale, fscale, time
    // (ns; args.get_time_ns may send a float), itrs; wall-clock time
    // limit; the workspace (first-pass columns per lane, escalation,
    // share of HBM) is the library's policy (capacity 0), the one the
    // bench measures
    r.so = cpd_search_opts{1.0, 0.0, r.k_moves, -1, 0, 0, 0, CPD_SEARCH_AUTO, 0.0, 0};
    if (!hscale.empty()) r.so.hscale = std::atof(hscale.c_str());
    if (!fscale.empty()) r.so.fscale = std::atof(fscale.c_str());
    if (!itrs.empty()) r.so.itrs = std::atoll(itrs.c_str());
    const double tn = std::atof(time.c_str());  // "": 0
    if (tn > 0) r.so.time_ns = (uint64_t)tn;
    return true;
}

// The answer line's 10 fields.  t_receive = query file read + parse + upload
// and sort on the GPU; t_search = the algorithm's device time (table-search:
// the walk kernel; cpd-search: the search passes + any table rebuild for new
// weights), the same meaning for both; t_astar = the A* passes alone (0 for
// table-search)
static std::string answer_line(bool search, const cpd_query_stats& st, const cpd_search_stats& ss,
                               double t_receive) {
    char buf[512];
    if (search)
        std::snprintf(buf, sizeof buf, "%llu,%llu,%llu,%llu,%llu,%llu,%llu,%lld,%lld,%lld",
                      (unsigned long long)ss.expanded, (unsigned long long)ss.inserted,
                      (unsigned long long)ss.touched, (unsigned long long)ss.updated,
                      (unsigned long long)ss.surplus, (unsigned long long)ss.plen,
                      (unsigned long long)ss.finished, (long long)(t_receive * 1e9),
                      (long long)(ss.kernel_ms * 1e6),
                      (long long)((ss.kernel_ms + ss.tables_ms) * 1e6));
    else
        std::snprintf(buf, sizeof buf, "%llu,0,0,0,0,%llu,%llu,%lld,0,%lld",
                      (unsigned long long)st.hops, (unsigned long long)st.hops,
                      (unsigned long long)st.finished, (long long)(t_receive * 1e9),
                      (long long)(st.kernel_ms * 1e6));
    return buf;
}

// <query file>.res of a "debug": true request: s t cost moves finished per
// query.  Written in place, and a file that cannot be opened is passed over.
static void write_debug_res(cpd_index* ix, const std::string& qfile, const std::vector<uint32_t>& s,
                            const std::vector<uint32_t>& t) {
    const size_t nq = s.size();
    std::vector<uint64_t> cost(nq);
    std::vector<uint32_t> hops(nq);
    std::vector<uint8_t> fin(nq);
    cli::check(cpd_query_fetch(ix, cost.data(), hops.data(), fin.data()), "fetch");
    std::FILE* f = std::fopen((qfile + ".res").c_str(), "w");
    if (!f) return;
    for (size_t i = 0; i < nq; ++i)
        std::fprintf(f, "%u %u %llu %u %u\n", s[i], t[i], (unsigned long long)cost[i], hops[i],
                     fin[i] == 1 ? 1u : 0u);
    std::fclose(f);
}

// The serve loop's state: which weights are active on the index, and the
// request buffers — allocated once and reused by every request, so that their
// pages stay mapped (a 1M-query file is ~14 MB of them).
struct Server {
    const Options& o;
    Loaded& L;
    std::string active_diff = "-";
    std::string active_sets;  // Costs, Timed: the diff list whose sets are loaded
    size_t active_nsets = 0;
    std::vector<uint32_t> s, t, cap;
    std::vector<uint64_t> dep, off;  // departures; path offsets

    Server(const Options& o, Loaded& L) : o(o), L(L) {}
    void set_weights(const std::string& diff);
    void assign(const Request& r, cpd_search_stats& ss);
    void compute(const Request& r, cpd_query_stats& st, cpd_search_stats& ss);
    std::string answer(const Request& r);  // the answer line; all zeros for a request that failed
};

// The request's weights, set when they are not the active ones: the one diff
// ("-": the .xy file's) on the index, or for Costs and Timed the list's sets,
// loaded beside (and independent of) the index's current weights.
void Server::set_weights(const std::string& diff) {
    if (!lists_diffs(o.mode)) {
        if (diff == active_diff) return;
        cli::check(cpd_index_set_weights(L.ix, diff == "-" ? nullptr : diff_weights(L, diff).data()),
                   "weights");
        active_diff = diff;
        return;
    }
    if (diff == active_sets) return;
    std::vector<const uint32_t*> sets;
    for (size_t p0 = 0; p0 <= diff.size();) {
        size_t p1 = diff.find(',', p0);
        if (p1 == std::string::npos) p1 = diff.size();
        const std::string name = diff.substr(p0, p1 - p0);
        if (name.empty()) throw std::runtime_error("empty name in diff list '" + diff + "'");
        if (sets.size() == CPD_MAX_WEIGHT_SETS)
            throw std::runtime_error("more than " + std::to_string(CPD_MAX_WEIGHT_SETS) +
                                     " diffs in '" + diff + "'");
        sets.push_back(name == "-" ? nullptr : diff_weights(L, name).data());
        p0 = p1 + 1;
    }
    active_sets.clear();  // a failed call leaves nothing active
    must(cpd_index_set_weight_sets(L.ix, (uint32_t)sets.size(), sets.data()));
    active_sets = diff;
    active_nsets = sets.size();
}

// An --assign request: the loop, its side files, and the answer line's sums
// from the last iteration's search.
void Server::assign(const Request& r, cpd_search_stats& ss) {
    const size_t nq = s.size();
    // the loop leaves w_{K+1} on the index: the next request sets its diff's
    // weights again, whatever its name
    active_diff.clear();
    cap.assign(L.g.m, (uint32_t)o.assign_cap);
    const uint32_t iters = (uint32_t)o.assign_iters;
    std::vector<std::string> lines;
    const double search_ms =
        o.step == Step::Line   ? run_assign<cpd_assign_line_iter>(cpd_query_assign_line, L.ix, r.so, cap,
                                                                  o.vdf, iters, lines)
        : o.step == Step::Conj ? run_assign<cpd_assign_conj_iter>(cpd_query_assign_conj, L.ix, r.so, cap,
                                                                  o.vdf, iters, lines)
                               : run_assign<cpd_assign_iter>(assign_msa, L.ix, r.so, cap, o.vdf, iters, lines);
    if (o.step == Step::Msa) write_loads(L.ix, r.qfile, L.g, 1);
    else write_flow(L.ix, r.qfile, L.g);
    write_assign(L.ix, r.qfile, L.g, lines);
    std::vector<uint32_t> cnt(5 * nq), plen(nq);
    std::vector<uint8_t> fin(nq);
    if (nq) cli::check(cpd_query_search_counters(L.ix, cnt.data()), "counters");
    cli::check(cpd_query_fetch(L.ix, nullptr, plen.data(), fin.data()), "fetch");
    uint64_t* sums[5] = {&ss.expanded, &ss.inserted, &ss.touched, &ss.updated, &ss.surplus};
    for (size_t q = 0; q < nq; ++q) {
        for (int k = 0; k < 5; ++k) *sums[k] += cnt[5 * q + k];
        if (fin[q] == 1) {
            ss.plen += plen[q];
            ss.finished++;
        } else if (fin[q] == 2) {
            ss.overflow++;
        }
    }
    ss.tables_ms = 0.0;
    ss.kernel_ms = search_ms;  // tables included
}

// The mode's call on the prepared queries, then its side files.
void Server::compute(const Request& r, cpd_query_stats& st, cpd_search_stats& ss) {
    cpd_index* ix = L.ix;
    const std::string& qf = r.qfile;
    switch (o.mode) {
    case Mode::Assign:
        assign(r, ss);
        break;
    case Mode::Search:
        must(cpd_query_search(ix, &r.so, &ss));
        break;
    case Mode::SearchPaths:
        off.resize(s.size() + 1);
        must(cpd_query_search_paths(ix, &r.so, 0, off.data(), &ss, nullptr));
        write_paths(ix, qf, s, t, off);
        break;
    case Mode::SearchLoads:
        must(cpd_query_search_loads(ix, &r.so, 0, nullptr, 0, &ss, nullptr));
        write_loads(ix, qf, L.g, 1);
        break;
    case Mode::Costs:
        must(cpd_query_costs(ix, r.k_moves, (uint32_t)o.slice_moves, &st));
        write_costs(ix, qf, s, t, o.slice_moves ? 1u : active_nsets);
        break;
    case Mode::Timed:
        must(cpd_query_timed(ix, r.k_moves, dep.empty() ? nullptr : dep.data(), (uint64_t)o.period,
                             nullptr, o.timed_loads ? CPD_TIMED_LOADS : 0u, &st));
        write_timed(ix, qf, s, t, dep);
        if (o.timed_loads) write_loads(ix, qf, L.g, active_nsets);
        break;
    case Mode::Loads:
        must(cpd_query_loads(ix, r.k_moves, nullptr, (uint32_t)o.load_slices,
                             (uint32_t)o.load_slice_moves, 0, &st));
        write_loads(ix, qf, L.g, (size_t)o.load_slices);
        break;
    case Mode::Paths:
        off.resize(s.size() + 1);
        must(cpd_query_paths(ix, r.k_moves, off.data(), &st));
        write_paths(ix, qf, s, t, off);
        break;
    case Mode::Run:
        must(cpd_query_run(ix, r.k_moves, &st));
        break;
    }
}

std::string Server::answer(const Request& r) {
    std::string line = "0,0,0,0,0,0,0,0,0,0";
    try {
        const double t0 = now();
        cpd::io::read_query_file(r.qfile, o.parse_threads, s, t);
        if (o.mode == Mode::Timed) read_departures(r.qfile, s.size(), dep);
        const double t_read = now() - t0;
        set_weights(r.diff);
        must(cpd_query_prepare(L.ix, s.data(), t.data(), (uint32_t)s.size()));
        const double t_receive = now() - t0;
        cpd_query_stats st{};
        cpd_search_stats ss{};
        compute(r, st, ss);
        if (ss.overflow)
            std::fprintf(stderr, "fifo_auto: %llu searches exceeded the workspace and stopped unfinished\n",
                         (unsigned long long)ss.overflow);
        if (r.debug && !lists_diffs(o.mode)) write_debug_res(L.ix, r.qfile, s, t);
        const bool search = is_search(o.mode);
        line = answer_line(search, st, ss, t_receive);
        if (o.verbose)  // the receive phase split (stderr: nothing reads stdout by then)
            std::fprintf(stderr, "fifo_auto-req: {\"queries\": %zu, \"read_parse_s\": %.6f, "
                         "\"prepare_s\": %.6f, \"compute_s\": %.6f}\n", s.size(), t_read,
                         t_receive - t_read, search ? ss.kernel_ms * 1e-3 : st.kernel_ms * 1e-3);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "fifo_auto: request failed: %s\n", e.what());
    }
    return line;
}

int main(int argc, char** argv) {
    Options o;
    if (const int rc = parse_options(argc, argv, o); rc >= 0) return rc;
    signal(SIGINT, on_signal);
    signal(SIGTERM, on_signal);
    signal(SIGPIPE, SIG_IGN);
    if (!make_fifo(o.fifo)) return 1;
    Loaded L;
    try {
        L = load(o);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "fifo_auto: %s\n", e.what());
        ::unlink(o.fifo.c_str());
        return 1;
    }
    Server server{o, L};
    while (!g_stop) {
        const std::string msg = read_all(o.fifo);
        if (g_stop) break;
        if (msg.empty()) continue;
        const std::string first = msg.substr(0, msg.find('\n'));
        if (first == "quit" || first == "exit") break;
        Request r;
        if (!parse_request(msg, r)) continue;
        const std::string line = server.answer(r);
        if (!write_answer(r.answer, line))
            std::fprintf(stderr, "fifo_auto: cannot write answer to %s\n", r.answer.c_str());
        if (o.once) break;
    }
    unload(L);
    return 0;
}

