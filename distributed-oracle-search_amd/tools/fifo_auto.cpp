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

// <query file>.paths: the walks' nodes, fetched and written in pieces of at
// most ~64M nodes (host memory stays bounded however long the paths are)
static void write_paths(cpd_index* ix, const std::string& qfile, const std::vector<uint32_t>& s,
                        const std::vector<uint32_t>& t, const std::vector<uint64_t>& off) {
    constexpr uint64_t kPiece = 64ull << 20;
    const size_t nq = s.size();
    std::vector<uint8_t> fin(nq);
    if (cpd_query_fetch(ix, nullptr, nullptr, fin.data()) != CPD_OK)
        throw std::runtime_error(cpd_last_error());
    const std::string path = qfile + ".paths", tmp = path + ".tmp";
    std::FILE* f = std::fopen(tmp.c_str(), "w");
    if (!f) throw std::runtime_error("cannot write " + tmp + ": " + std::strerror(errno));
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
        if (cpd_query_paths_fetch(ix, (uint32_t)q0, (uint32_t)(q1 - q0), nodes.data()) != CPD_OK) {
            std::fclose(f);
            ::unlink(tmp.c_str());
            throw std::runtime_error(cpd_last_error());
        }
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
    ok = std::fclose(f) == 0 && ok;
    if (!ok || ::rename(tmp.c_str(), path.c_str()) != 0) {
        ::unlink(tmp.c_str());
        throw std::runtime_error("cannot write " + path);
    }
}

// <query file>.res of a --costs request: s t moves finished cost_0 ... per query
static void write_costs(cpd_index* ix, const std::string& qfile, const std::vector<uint32_t>& s,
                        const std::vector<uint32_t>& t, size_t cols) {
    const size_t nq = s.size();
    std::vector<uint64_t> costs(nq * cols);
    std::vector<uint32_t> hops(nq);
    std::vector<uint8_t> fin(nq);
    if (cpd_query_costs_fetch(ix, costs.data(), hops.data(), fin.data()) != CPD_OK)
        throw std::runtime_error(cpd_last_error());
    const std::string path = qfile + ".res", tmp = path + ".tmp";
    std::FILE* f = std::fopen(tmp.c_str(), "w");
    if (!f) throw std::runtime_error("cannot write " + tmp + ": " + std::strerror(errno));
    bool ok = true;
    for (size_t q = 0; q < nq && ok; ++q) {
        ok = std::fprintf(f, "%u %u %u %u", s[q], t[q], hops[q], fin[q] == 1 ? 1u : 0u) > 0;
        for (size_t j = 0; j < cols && ok; ++j)
            ok = std::fprintf(f, " %llu", (unsigned long long)costs[q * cols + j]) > 0;
        ok = ok && std::fputc('\n', f) != EOF;
    }
    ok = std::fclose(f) == 0 && ok;
    if (!ok || ::rename(tmp.c_str(), path.c_str()) != 0) {
        ::unlink(tmp.c_str());
        throw std::runtime_error("cannot write " + path);
    }
}

// <query file>.loads: edge from to load_0 ... per edge with any non-zero value
static void write_load_values(const std::string& qfile, const cpd::io::XYGraph& g, size_t slices,
                              const std::vector<uint64_t>& loads) {
    const std::string path = qfile + ".loads", tmp = path + ".tmp";
    std::FILE* f = std::fopen(tmp.c_str(), "w");
    if (!f) throw std::runtime_error("cannot write " + tmp + ": " + std::strerror(errno));
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
    ok = std::fclose(f) == 0 && ok;
    if (!ok || ::rename(tmp.c_str(), path.c_str()) != 0) {
        ::unlink(tmp.c_str());
        throw std::runtime_error("cannot write " + path);
    }
}

// <query file>.loads of a --loads request: the resident table
static void write_loads(cpd_index* ix, const std::string& qfile, const cpd::io::XYGraph& g,
                        size_t slices) {
    std::vector<uint64_t> loads(slices * g.m);
    if (cpd_query_loads_fetch(ix, loads.data()) != CPD_OK)
        throw std::runtime_error(cpd_last_error());
    write_load_values(qfile, g, slices, loads);
}

// <query file>.loads of an --assign --step line request: the flow's volumes
static void write_flow(cpd_index* ix, const std::string& qfile, const cpd::io::XYGraph& g) {
    std::vector<uint64_t> x(g.m);
    if (cpd_index_flow_fetch(ix, x.data()) != CPD_OK) throw std::runtime_error(cpd_last_error());
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
    std::string path = qfile + ".assign", tmp = path + ".tmp";
    std::FILE* f = std::fopen(tmp.c_str(), "w");
    if (!f) throw std::runtime_error("cannot write " + tmp + ": " + std::strerror(errno));
    bool ok = true;
    for (size_t k = 0; k < lines.size() && ok; ++k)
        ok = std::fprintf(f, "%zu %s\n", k + 1, lines[k].c_str()) > 0;
    ok = std::fclose(f) == 0 && ok;
    if (!ok || ::rename(tmp.c_str(), path.c_str()) != 0) {
        ::unlink(tmp.c_str());
        throw std::runtime_error("cannot write " + path);
    }
    std::vector<uint32_t> w(g.m);
    if (cpd_index_get_weights(ix, w.data()) != CPD_OK) throw std::runtime_error(cpd_last_error());
    path = qfile + ".diff";
    tmp = path + ".tmp";
    cpd::io::write_diff(tmp, g, w);
    if (::rename(tmp.c_str(), path.c_str()) != 0) {
        ::unlink(tmp.c_str());
        throw std::runtime_error("cannot write " + path);
    }
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
    if (loop(ix, &so, 0, nullptr, cap.data(), &vdf, iters, it.data(), &made) != CPD_OK)
        throw std::runtime_error(cpd_last_error());
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
    if (cpd_query_timed_fetch(ix, cost.data(), hops.data(), fin.data()) != CPD_OK)
        throw std::runtime_error(cpd_last_error());
    const std::string path = qfile + ".res", tmp = path + ".tmp";
    std::FILE* f = std::fopen(tmp.c_str(), "w");
    if (!f) throw std::runtime_error("cannot write " + tmp + ": " + std::strerror(errno));
    bool ok = true;
    for (size_t q = 0; q < nq && ok; ++q)
        ok = std::fprintf(f, "%u %u %u %u %llu %llu\n", s[q], t[q], hops[q], fin[q] == 1 ? 1u : 0u,
                          (unsigned long long)(dep.empty() ? 0 : dep[q]),
                          (unsigned long long)cost[q]) > 0;
    ok = std::fclose(f) == 0 && ok;
    if (!ok || ::rename(tmp.c_str(), path.c_str()) != 0) {
        ::unlink(tmp.c_str());
        throw std::runtime_error("cannot write " + path);
    }
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

int main(int argc, char** argv) {
    cli::Args a(argc, argv);
    const auto& inputs = a.list("input");
    std::string method = a.str_any({"partmethod", "partition"});
    long long key = a.num("partkey", -1), wid = a.num("workerid", -1), W = a.num("maxworker", -1);
    std::string alg = a.str("alg", "table-search");
    if (inputs.empty() || method.empty() || key <= 0 || wid < 0 || W <= 0 || wid >= W) {
        std::fprintf(stderr,
                     "usage: fifo_auto --input X.xy [DIFF] --partmethod {div|mod} --partkey K "
                     "--workerid I --maxworker W --outdir D --alg table-search|cpd-search\n"
                     "       [--paths]  table-search only: answer through cpd_query_paths and "
                     "write every\n"
                     "                  walk's nodes to <query file>.paths, one line per query:\n"
                     "                  s t finished n v0 ... v(n-1)\n"
                     "       [--search-paths]  cpd-search only: answer through "
                     "cpd_query_search_paths and\n"
                     "                  write every route's nodes to <query file>.paths, same "
                     "format\n"
                     "       [--search-loads]  cpd-search only: answer through "
                     "cpd_query_search_loads (demand 1\n"
                     "                  per query) and write every loaded edge of the routes "
                     "found to\n"
                     "                  <query file>.loads: edge from to load\n"
                     "       [--costs [--slice-moves S]]  table-search only: the request's diff "
                     "field may list\n"
                     "                  up to 8 diffs (\"-,a.diff,b.diff\"); one walk costs every "
                     "query under each\n"
                     "                  (cpd_query_costs) and <query file>.res gets, per query:\n"
                     "                  s t moves finished cost_0 ... cost_{C-1}\n"
                     "                  (with --slice-moves S one cost: move h under diff "
                     "min(h / S, last));\n"
                     "                  \"debug\": true in a request adds nothing: .res is the "
                     "costs file\n"
                     "       [--loads [--load-slices K --load-slice-moves S]]  table-search only: "
                     "answer through\n"
                     "                  cpd_query_loads (demand 1 per query) and write every "
                     "loaded edge to\n"
                     "                  <query file>.loads: edge from to load_0 ... load_{K-1}\n"
                     "                  (K slices: move h counts in slice min(h / S, K - 1))\n"
                     "       [--timed P [--loads]]  table-search only: answer through "
                     "cpd_query_timed; the\n"
                     "                  request's diff field lists up to 8 diffs, diff j the "
                     "network during clock\n"
                     "                  time [j P, (j + 1) P); departures from <query file>.dep "
                     "(one per query\n"
                     "                  line; absent: 0); <query file>.res gets, per query:\n"
                     "                  s t moves finished depart cost\n"
                     "                  (with --loads <query file>.loads has one column per "
                     "diff)\n"
                     "       [--assign K --capacity C [--vdf A/B^P]]  cpd-search only: answer "
                     "through\n"
                     "                  cpd_query_assign (K iterations, demand 1 per query, every "
                     "edge at capacity C,\n"
                     "                  delay w0 (1 + A/B (x/C)^P), default 3/20^4); writes <query "
                     "file>.loads,\n"
                     "                  .assign (k finished sptt tstt moves changed) and .diff (the "
                     "final weights)\n"
                     "       [--step msa|line|conj]  with --assign: msa (default) as above; line answers "
                     "through\n"
                     "                  cpd_query_assign_line (the line-search step): .assign lines "
                     "end in\n"
                     "                  lambda g0 xw0, .loads holds the final flow's volumes; conj "
                     "answers through\n"
                     "                  cpd_query_assign_conj (the conjugate step): .assign lines "
                     "end in lambda gy xw0 alpha\n");
        return 2;
    }
    // table-search (make_fifos.py:20) or the CPD-heuristic search
    // (cpd_query_search; args.py:29-57)
    const bool search = alg == "cpd-search" || alg == "cpd_search";
    if (alg != "table-search" && !search) {
        std::fprintf(stderr, "fifo_auto: --alg must be table-search or cpd-search (got '%s')\n",
                     alg.c_str());
        return 2;
    }
    const bool paths = a.has("paths");
    if (paths && search) {
        std::fprintf(stderr, "fifo_auto: --paths needs --alg table-search (the paths of a "
                             "cpd-search are extracted with --search-paths)\n");
        return 2;
    }
    const bool search_paths = a.has("search-paths");
    if (search_paths && !search) {
        std::fprintf(stderr, "fifo_auto: --search-paths needs --alg cpd-search (the walks of a "
                             "table-search are extracted with --paths)\n");
        return 2;
    }
    const bool costs = a.has("costs");
    if (costs && (search || paths)) {
        std::fprintf(stderr, "fifo_auto: --costs needs --alg table-search without --paths (a "
                             "cpd-search's route depends on the weights; --paths answers through "
                             "cpd_query_paths)\n");
        return 2;
    }
    const long long slice_moves = a.num("slice-moves", 0);
    if ((slice_moves && !costs) || slice_moves < 0 || slice_moves > 0xFFFFFFFFll) {
        std::fprintf(stderr, "fifo_auto: --slice-moves S needs --costs and 0 <= S < 2^32\n");
        return 2;
    }
    const bool loads = a.has("loads");
    if (loads && (search || paths || costs)) {
        std::fprintf(stderr, "fifo_auto: --loads needs --alg table-search without --paths or "
                             "--costs (a cpd-search's route is not the walk's: --search-loads loads "
                             "it; --paths and --costs "
                             "answer through cpd_query_paths and cpd_query_costs)\n");
        return 2;
    }
    const bool timed = a.has("timed");
    if (timed && (search || paths || costs || a.has("load-slices") || a.has("load-slice-moves"))) {
        std::fprintf(stderr, "fifo_auto: --timed needs --alg table-search without --paths, --costs, "
                             "--load-slices or --load-slice-moves (a cpd-search's route is not the "
                             "walk's; --paths and --costs answer through cpd_query_paths and "
                             "cpd_query_costs; a timed walk's load planes are its diffs)\n");
        return 2;
    }
    const long long period = a.num("timed", 0);
    if (timed && (period < 1 || period > (1ll << 60))) {
        std::fprintf(stderr, "fifo_auto: --timed P needs 1 <= P <= 2^60\n");
        return 2;
    }
    const bool search_loads = a.has("search-loads");
    if (search_loads && (!search || search_paths || a.has("load-slices") || a.has("load-slice-moves"))) {
        std::fprintf(stderr, "fifo_auto: --search-loads needs --alg cpd-search without --search-paths, "
                             "--load-slices or --load-slice-moves (the walks of a table-search are "
                             "loaded with --loads; --search-paths answers through "
                             "cpd_query_search_paths; a search loads one plane)\n");
        return 2;
    }
    const long long load_slices = a.num("load-slices", 1), load_slice_moves = a.num("load-slice-moves", 0);
    if (((a.has("load-slices") || a.has("load-slice-moves")) && !loads) || load_slices < 1 ||
        load_slices > (long long)CPD_MAX_LOAD_SLICES || load_slice_moves < 0 ||
        load_slice_moves > 0xFFFFFFFFll || (load_slices == 1) != (load_slice_moves == 0)) {
        std::fprintf(stderr, "fifo_auto: --load-slices K --load-slice-moves S need --loads, 2 <= K "
                             "<= %u and 0 < S < 2^32 (both or neither)\n", CPD_MAX_LOAD_SLICES);
        return 2;
    }
    const bool assign = a.has("assign");
    if (assign && (!search || search_paths || search_loads || loads || timed)) {
        std::fprintf(stderr, "fifo_auto: --assign needs --alg cpd-search without --search-paths, "
                             "--search-loads, --loads or --timed (the loop answers through "
                             "cpd_query_assign and writes the loads itself)\n");
        return 2;
    }
    const long long assign_iters = a.num("assign", 0), assign_cap = a.num("capacity", 0);
    cpd_vdf vdf{3, 20, 4, 1};
    {
        const std::string v = a.str("vdf", "3/20^4");
        unsigned an = 0, ad = 0, pw = 0;
        char tail = 0;
        const bool ok = std::sscanf(v.c_str(), "%u/%u^%u%c", &an, &ad, &pw, &tail) == 3 &&
                        an <= 65535u && ad >= 1u && ad <= 65535u && pw >= 1u && pw <= 4u;
        if ((a.has("vdf") || a.has("capacity")) && !assign) {
            std::fprintf(stderr, "fifo_auto: --capacity and --vdf need --assign\n");
            return 2;
        }
        if (assign && (!ok || assign_iters < 1 || assign_iters > 65535 || assign_cap < 1 ||
                       assign_cap > 0xFFFFFFFFll)) {
            std::fprintf(stderr, "fifo_auto: --assign K --capacity C [--vdf A/B^P] need 1 <= K <= "
                                 "65535, 1 <= C < 2^32, A <= 65535, 1 <= B <= 65535 and 1 <= P <= 4\n");
            return 2;
        }
        vdf = cpd_vdf{an, ad, pw, 1};
    }
    const std::string step = a.str("step", "msa");
    if ((a.has("step") && !assign) || (step != "msa" && step != "line" && step != "conj")) {
        std::fprintf(stderr, "fifo_auto: --step msa|line|conj needs --assign\n");
        return 2;
    }
    const bool step_line = step == "line", step_conj = step == "conj";
    int mcode = cli::method_code(method);
    std::string xy = inputs[0];
    std::string outdir = a.str("outdir", ".");
    std::string fifo = a.str("fifo", "/tmp/worker" + std::to_string(wid) + ".fifo");
    bool once = a.has("once");
    // threads parsing a request's query file (a 1M-query file is ~14 MB)
    const int parse_threads = (int)a.num("parse-threads", 16);
    const bool verbose = a.has("verbose");
    signal(SIGINT, on_signal);
    signal(SIGTERM, on_signal);
    signal(SIGPIPE, SIG_IGN);

    // The request FIFO exists before the (possibly long) index load: a request
    // sent meanwhile blocks in its writer's open() until the loop below reads
    // it, instead of `cat <<CONF > fifo` creating a regular file there.  A
    // non-FIFO left at the path (such a file from an earlier run) is replaced.
    {
        struct stat st;
        if (::lstat(fifo.c_str(), &st) == 0 && !S_ISFIFO(st.st_mode)) ::unlink(fifo.c_str());
        if (::mkfifo(fifo.c_str(), 0666) != 0 && errno != EEXIST) {
            std::fprintf(stderr, "fifo_auto: mkfifo %s: %s\n", fifo.c_str(), std::strerror(errno));
            return 1;
        }
        if (::lstat(fifo.c_str(), &st) != 0 || !S_ISFIFO(st.st_mode)) {
            std::fprintf(stderr, "fifo_auto: %s is not a FIFO\n", fifo.c_str());
            return 1;
        }
    }

    cpd_index* ix = nullptr;
    cpd_graph* dg = nullptr;
    cpd_plan* plan = nullptr;
    cpd::io::XYGraph g;
    std::map<std::string, std::vector<uint32_t>> diff_cache;
    std::string active_diff = "-";
    std::string active_sets;  // --costs: the diff list whose sets are loaded
    size_t active_nsets = 0;
    int device = -1;
    bool arena = false;
    try {
        double t0 = now();
        // This worker's buckets, headers first (targets, run counts or
        // offsets): DOSCPD02/03 (compact move tables, what make_cpd_auto
        // writes by default) or DOSCPD01 (run words).  The node count comes
        // from the order file make_cpd_auto wrote beside them; the graph's
        // fingerprint is checked once the .xy is read.
        const uint32_t n0 = cpd::io::read_order_n(cpd::io::order_path(outdir, xy));
        uint32_t nb = 0;
        cli::check(cpd_partition_nbuckets(n0, mcode, (uint32_t)key, &nb), "buckets");
        std::vector<std::string> paths;
        std::vector<int> formats;
        std::vector<cpd::io::CpdBucket> heads;
        std::vector<cpd::io::MoveBucket> mheads;
        std::vector<uint32_t> targets;
        uint64_t total_runs = 0, compact_bytes = 0;
        uint32_t move_bits = 0;  // the compact rows' width (0: some bucket holds run words)
        bool all_compact = true;
        for (uint32_t b = 0; b < nb; ++b) {
            if (b % (uint32_t)W != (uint32_t)wid) continue;
            paths.push_back(cpd::io::bucket_path(outdir, xy, method, (uint32_t)key, b));
            formats.push_back(cpd::io::bucket_format(paths.back()));
            if (formats.back() == 1) {
                heads.push_back(cpd::io::read_bucket_head(paths.back()));
                mheads.emplace_back();
                const auto& bk = heads.back();
                targets.insert(targets.end(), bk.targets.begin(), bk.targets.end());
                total_runs += bk.offsets.back();
                all_compact = false;
            } else {
                mheads.push_back(cpd::io::read_move_bucket_head(paths.back()));
                heads.emplace_back();
                const auto& bk = mheads.back();
                if (bk.n != n0) throw std::runtime_error("bucket " + std::to_string(b) + " has another node count");
                targets.insert(targets.end(), bk.targets.begin(), bk.targets.end());
                total_runs += bk.total_runs;
                compact_bytes += 4ull * bk.words * bk.targets.size();
                move_bits = bk.bits;
            }
        }
        // The device side starts now, on a thread, beside the host reads
        // (VERDICT r04 item 7): the first HIP call and, for compact buckets,
        // the dense index's HBM committed as an arena (nrows x n padded to
        // 2048 columns x bits / 8 bytes: committing fresh HBM costs about a
        // second per 30 GB) that cpd_index_create_empty then carves.
        int ndev = 0;
        double t_dev = 0.0;
        int dev_rc = CPD_OK;
        std::string dev_err;
        std::thread dev_thr([&] {
            const double td = now();
            dev_rc = cpd_device_count(&ndev);
            if (dev_rc == CPD_OK && ndev > 0) {
                device = (int)a.num("device", wid % ndev);
                if (all_compact && !targets.empty() && move_bits) {
                    const uint64_t npad = (n0 + 2047ull) / 2048ull * 2048ull;
                    const uint64_t bytes = (uint64_t)targets.size() * (npad * move_bits / 32ull) * 4ull;
                    // only for an index that will be dense (--index rle keeps
                    // runs; auto takes tables when the runs weigh more — the
                    // index's own test): an unused arena would hold HBM the
                    // search workspace is sized from
                    const std::string im0 = a.str("index", "auto");
                    const bool dense = im0 == "dense" || (im0 != "rle" && 4ull * total_runs > bytes);
                    if (dense) arena = cpd_device_arena(device, bytes + (1ull << 20), 0) == CPD_OK;
                }
            }
            if (dev_rc != CPD_OK) dev_err = cpd_last_error();
            t_dev = now() - td;
        });
        struct Join {
            std::thread& t;
            ~Join() {
                if (t.joinable()) t.join();
            }
        } join{dev_thr};
        g = cpd::io::read_xy(xy);
        uint64_t fp = cpd::io::graph_fingerprint(g.n, g.row_ptr.data(), g.dst.data(), g.w.data());
        if (inputs.size() > 1) diff_cache[inputs[1]] = cpd::io::read_diff(inputs[1], g);
        cpd_plan_opts o{};
        o.no_hierarchy = 1;  // queries need the CSR + column order only
        cli::check(cpd_plan_create(g.row_ptr.data(), g.dst.data(), g.w.data(), g.n, g.m, &o, &plan),
                   "plan");
        std::vector<uint32_t> order(g.n);
        cli::check(cpd_plan_order(plan, order.data()), "order");
        std::vector<uint32_t> stored = cpd::io::read_order(cpd::io::order_path(outdir, xy), fp);
        if (stored != order) throw std::runtime_error("stored column order differs from this build's");
        for (size_t k = 0; k < paths.size(); ++k) {
            const bool rle = formats[k] == 1;
            const uint64_t bfp = rle ? heads[k].fingerprint : mheads[k].fingerprint;
            const uint32_t bkey = rle ? heads[k].key : mheads[k].key;
            const uint32_t bmethod = rle ? heads[k].method : mheads[k].method;
            if (bfp != fp || bkey != (uint32_t)key || bmethod != (uint32_t)mcode)
                throw std::runtime_error(paths[k] + " was built for another graph/partition");
        }
        const double t_graph0 = now();
        dev_thr.join();
        const double t_devwait = now() - t_graph0;
        if (dev_rc != CPD_OK) throw std::runtime_error("device: " + dev_err);
        if (ndev == 0) throw std::runtime_error("no GPU visible (this build has no CPU path)");
        cli::check(cpd_graph_create(plan, device, &dg), "graph upload");
        // then the rows, streamed in pieces of <= kPiece words (a longer row
        // alone): a dense index never holds the worker's runs in HBM or RAM
        const std::string im = a.str("index", "auto");
        const int imode = im == "rle" ? CPD_INDEX_RLE : im == "dense" ? CPD_INDEX_DENSE : CPD_INDEX_AUTO;
        cli::check(cpd_index_create_empty(dg, targets.data(), (uint32_t)targets.size(), imode,
                                          total_runs, &ix),
                   "index");
        const double t_rows0 = now();
        constexpr uint64_t kPiece = 64ull << 20;  // 256 MB
        std::vector<uint32_t> buf;
        std::vector<uint64_t> rel;
        // compact buckets: pieces read into two page-locked buffers by a
        // reader thread while the previous piece is appended (uploaded)
        uint32_t* pin[2] = {nullptr, nullptr};
        uint64_t pin_bytes = 0;
        const int read_threads = (int)a.num("read-threads", 8);
        for (size_t k = 0; k < paths.size(); ++k) {
            if (formats[k] == 2) {
                const auto& mh = mheads[k];
                const uint32_t nr = (uint32_t)mh.targets.size();
                if (!nr) continue;
                const uint32_t per = (uint32_t)std::min<uint64_t>(nr, std::max<uint64_t>(1, kPiece / mh.words));
                if (4ull * mh.words * per > pin_bytes) {  // grown for this bucket's pieces
                    for (auto& p : pin) {
                        cpd_host_free(p);
                        void* q = nullptr;
                        cli::check(cpd_host_alloc(4ull * mh.words * per, &q), "pinned buffer");
                        p = static_cast<uint32_t*>(q);
                    }
                    pin_bytes = 4ull * mh.words * per;
                }
                auto read = [&, k, per, nr](uint32_t r0, int slot) {
                    cpd::io::read_move_bucket_rows(paths[k], mheads[k], r0, std::min(per, nr - r0), pin[slot],
                                                   read_threads);
                };
                std::future<void> rd = std::async(std::launch::async, read, 0u, 0);
                for (uint32_t r0 = 0, i = 0; r0 < nr; r0 += per, ++i) {
                    rd.get();  // piece i is in pin[i & 1] (a read error is rethrown here)
                    if (r0 + per < nr) rd = std::async(std::launch::async, read, r0 + per, (int)((i + 1) & 1u));
                    const int rc = cpd_index_append_moves(ix, std::min(per, nr - r0), mh.bits, pin[i & 1u]);
                    if (rc != CPD_OK) {
                        if (rd.valid()) rd.wait();
                        cli::check(rc, "index rows");
                    }
                }
                continue;
            }
            const auto& off = heads[k].offsets;
            const uint32_t nr = (uint32_t)heads[k].targets.size();
            for (uint32_t r0 = 0; r0 < nr;) {
                uint32_t r1 = r0 + 1;
                while (r1 < nr && off[r1 + 1] - off[r0] <= kPiece) ++r1;
                buf.resize(off[r1] - off[r0]);
                cpd::io::read_bucket_runs(paths[k], heads[k], off[r0], buf.size(), buf.data());
                rel.resize(r1 - r0 + 1);
                for (uint32_t i = r0; i <= r1; ++i) rel[i - r0] = off[i] - off[r0];
                cli::check(cpd_index_append_rows(ix, r1 - r0, rel.data(), buf.data()), "index rows");
                r0 = r1;
            }
        }
        for (auto p : pin) cpd_host_free(p);
        const double t_rows = now() - t_rows0;
        int mode = 0;
        cli::check(cpd_index_get_mode(ix, &mode), "index mode");
        // one machine-readable line (bench.py's full-build leg reads it)
        std::printf("fifo_auto-json: {\"worker\": %lld, \"rows\": %zu, \"runs\": %llu, "
                    "\"index\": \"%s\", \"compact_bytes\": %llu, \"read_plan_s\": %.3f, "
                    "\"device_s\": %.3f, \"device_wait_s\": %.3f, \"arena\": %s, "
                    "\"graph_s\": %.3f, \"rows_s\": %.3f, \"ready_s\": %.3f}\n",
                    wid, targets.size(), (unsigned long long)total_runs,
                    mode == CPD_INDEX_DENSE ? "dense" : "rle", (unsigned long long)compact_bytes,
                    t_graph0 - t0, t_dev, t_devwait, arena ? "true" : "false",
                    t_rows0 - t_graph0, t_rows, now() - t0);
        std::printf("fifo_auto: worker %lld: %zu rows, %llu runs (%s index) on device %d, ready in "
                    "%.3fs; listening on %s\n",
                    wid, targets.size(), (unsigned long long)total_runs,
                    mode == CPD_INDEX_DENSE ? "dense" : "rle", device, now() - t0, fifo.c_str());
        std::fflush(stdout);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "fifo_auto: %s\n", e.what());
        ::unlink(fifo.c_str());
        return 1;
    }

    while (!g_stop) {
        std::string msg = read_all(fifo);
        if (g_stop) break;
        if (msg.empty()) continue;
        size_t nl = msg.find('\n');
        std::string conf = msg.substr(0, nl);
        if (conf == "quit" || conf == "exit") break;
        std::string rest = nl == std::string::npos ? "" : msg.substr(nl + 1);
        char qfile[4096] = {0}, answer[4096] = {0}, dname[4096] = {0};
        int got = std::sscanf(rest.c_str(), "%4095s %4095s %4095s", qfile, answer, dname);
        if (got < 2) {
            std::fprintf(stderr, "fifo_auto: malformed request: %s\n", msg.c_str());
            continue;
        }
        std::string diff = got >= 3 ? dname : "-";
        int k_moves = -1;
        std::string km = json_field(conf, "k_moves");
        if (!km.empty()) k_moves = std::atoi(km.c_str());
        bool debug = json_field(conf, "debug") == "true";
        // cpd-search knobs (process_query.py:149-160): hscale, fscale, time
        // (ns; args.get_time_ns may send a float), itrs; wall-clock time
        // limit; the workspace (first-pass columns per lane, escalation,
        // share of HBM) is the library's policy (capacity 0), the one the
        // bench measures
        cpd_search_opts so{1.0, 0.0, k_moves, -1, 0, 0, 0, CPD_SEARCH_AUTO, 0.0, 0};
        if (!json_field(conf, "hscale").empty()) so.hscale = std::atof(json_field(conf, "hscale").c_str());
        if (!json_field(conf, "fscale").empty()) so.fscale = std::atof(json_field(conf, "fscale").c_str());
        if (!json_field(conf, "itrs").empty()) so.itrs = std::atoll(json_field(conf, "itrs").c_str());
        if (!json_field(conf, "time").empty()) {
            const double tn = std::atof(json_field(conf, "time").c_str());
            so.time_ns = tn > 0 ? (uint64_t)tn : 0;
        }
        std::string line = "0,0,0,0,0,0,0,0,0,0";
        try {
            double t0 = now();
            // kept across requests: their pages stay mapped
            static std::vector<uint32_t> s, t;
            cpd::io::read_query_file(qfile, parse_threads, s, t);
            static std::vector<uint64_t> dep;
            if (timed) read_departures(qfile, s.size(), dep);
            const double t_read = now() - t0;
            if (costs || timed) {
                // the diff field is a list: its sets, loaded beside (and
                // independent of) the index's current weights
                if (diff != active_sets) {
                    std::vector<const uint32_t*> sets;
                    for (size_t p0 = 0; p0 <= diff.size();) {
                        size_t p1 = diff.find(',', p0);
                        if (p1 == std::string::npos) p1 = diff.size();
                        const std::string name = diff.substr(p0, p1 - p0);
                        if (name.empty()) throw std::runtime_error("empty name in diff list '" + diff + "'");
                        if (sets.size() == CPD_MAX_WEIGHT_SETS)
                            throw std::runtime_error("more than " + std::to_string(CPD_MAX_WEIGHT_SETS) +
                                                     " diffs in '" + diff + "'");
                        if (name == "-") {
                            sets.push_back(nullptr);
                        } else {
                            auto it = diff_cache.find(name);
                            if (it == diff_cache.end())
                                it = diff_cache.emplace(name, cpd::io::read_diff(name, g)).first;
                            sets.push_back(it->second.data());
                        }
                        p0 = p1 + 1;
                    }
                    active_sets.clear();
                    if (cpd_index_set_weight_sets(ix, (uint32_t)sets.size(), sets.data()) != CPD_OK)
                        throw std::runtime_error(cpd_last_error());
                    active_sets = diff;
                    active_nsets = sets.size();
                }
            } else if (diff != active_diff) {
                if (diff == "-" ) {
                    cli::check(cpd_index_set_weights(ix, nullptr), "weights");
                } else {
                    auto it = diff_cache.find(diff);
                    if (it == diff_cache.end())
                        it = diff_cache.emplace(diff, cpd::io::read_diff(diff, g)).first;
                    cli::check(cpd_index_set_weights(ix, it->second.data()), "weights");
                }
                active_diff = diff;
            }
            const size_t nq = s.size();
            int rc = cpd_query_prepare(ix, s.data(), t.data(), (uint32_t)nq);
            if (rc != CPD_OK) throw std::runtime_error(cpd_last_error());
            double t_receive = now() - t0;
            cpd_query_stats st{};
            cpd_search_stats ss{};
            if (assign) {
                // the loop leaves w_{K+1} on the index: the next request sets
                // its diff's weights again, whatever its name
                active_diff.clear();
                static std::vector<uint32_t> cap;
                cap.assign(g.m, (uint32_t)assign_cap);
                const uint32_t iters = (uint32_t)assign_iters;
                std::vector<std::string> lines;
                const double search_ms =
                    step_line   ? run_assign<cpd_assign_line_iter>(cpd_query_assign_line, ix, so, cap,
                                                                   vdf, iters, lines)
                    : step_conj ? run_assign<cpd_assign_conj_iter>(cpd_query_assign_conj, ix, so, cap,
                                                                   vdf, iters, lines)
                                : run_assign<cpd_assign_iter>(assign_msa, ix, so, cap, vdf, iters, lines);
                if (step_line || step_conj) write_flow(ix, qfile, g);
                else write_loads(ix, qfile, g, 1);
                write_assign(ix, qfile, g, lines);
                // the answer line's sums, from the last iteration's search
                std::vector<uint32_t> cnt(5 * nq), plen(nq);
                std::vector<uint8_t> fin(nq);
                if (nq) cli::check(cpd_query_search_counters(ix, cnt.data()), "counters");
                cli::check(cpd_query_fetch(ix, nullptr, plen.data(), fin.data()), "fetch");
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
                if (ss.overflow)
                    std::fprintf(stderr, "fifo_auto: %llu searches exceeded the workspace and stopped unfinished\n",
                                 (unsigned long long)ss.overflow);
            } else if (search) {
                static std::vector<uint64_t> spoff;
                if (search_paths) {
                    spoff.resize(nq + 1);
                    rc = cpd_query_search_paths(ix, &so, 0, spoff.data(), &ss, nullptr);
                } else if (search_loads) {
                    rc = cpd_query_search_loads(ix, &so, 0, nullptr, 0, &ss, nullptr);
                } else {
                    rc = cpd_query_search(ix, &so, &ss);
                }
                if (rc != CPD_OK) throw std::runtime_error(cpd_last_error());
                if (search_paths) write_paths(ix, qfile, s, t, spoff);
                if (search_loads) write_loads(ix, qfile, g, 1);
                if (ss.overflow)
                    std::fprintf(stderr, "fifo_auto: %llu searches exceeded the workspace and stopped unfinished\n",
                                 (unsigned long long)ss.overflow);
            } else if (costs) {
                rc = cpd_query_costs(ix, k_moves, (uint32_t)slice_moves, &st);
                if (rc != CPD_OK) throw std::runtime_error(cpd_last_error());
                write_costs(ix, qfile, s, t, slice_moves ? 1u : active_nsets);
            } else if (timed) {
                rc = cpd_query_timed(ix, k_moves, dep.empty() ? nullptr : dep.data(),
                                     (uint64_t)period, nullptr, loads ? CPD_TIMED_LOADS : 0u, &st);
                if (rc != CPD_OK) throw std::runtime_error(cpd_last_error());
                write_timed(ix, qfile, s, t, dep);
                if (loads) write_loads(ix, qfile, g, active_nsets);
            } else if (loads) {
                rc = cpd_query_loads(ix, k_moves, nullptr, (uint32_t)load_slices,
                                     (uint32_t)load_slice_moves, 0, &st);
                if (rc != CPD_OK) throw std::runtime_error(cpd_last_error());
                write_loads(ix, qfile, g, (size_t)load_slices);
            } else if (paths) {
                static std::vector<uint64_t> poff;
                poff.resize(nq + 1);
                rc = cpd_query_paths(ix, k_moves, poff.data(), &st);
                if (rc != CPD_OK) throw std::runtime_error(cpd_last_error());
                write_paths(ix, qfile, s, t, poff);
            } else {
                rc = cpd_query_run(ix, k_moves, &st);
                if (rc != CPD_OK) throw std::runtime_error(cpd_last_error());
            }
            if (debug && !costs && !timed) {
                std::vector<uint64_t> cost(nq);
                std::vector<uint32_t> hops(nq);
                std::vector<uint8_t> fin(nq);
                cli::check(cpd_query_fetch(ix, cost.data(), hops.data(), fin.data()), "fetch");
                std::string res = std::string(qfile) + ".res";
                if (std::FILE* f = std::fopen(res.c_str(), "w")) {
                    for (size_t i = 0; i < nq; ++i)
                        std::fprintf(f, "%u %u %llu %u %u\n", s[i], t[i], (unsigned long long)cost[i],
                                     hops[i], fin[i] == 1 ? 1u : 0u);
                    std::fclose(f);
                }
            }
            // t_receive = query file read + parse + upload and sort on the
            // GPU; t_search = the algorithm's device time (table-search: the
            // walk kernel; cpd-search: the search passes + any table rebuild
            // for new weights), the same meaning for both; t_astar = the A*
            // passes alone (0 for table-search)
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
            line = buf;
            if (verbose)  // the receive phase split (stderr: nothing reads stdout by then)
                std::fprintf(stderr, "fifo_auto-req: {\"queries\": %zu, \"read_parse_s\": %.6f, "
                             "\"prepare_s\": %.6f, \"compute_s\": %.6f}\n", nq, t_read,
                             t_receive - t_read, search ? ss.kernel_ms * 1e-3 : st.kernel_ms * 1e-3);
        } catch (const std::exception& e) {
            std::fprintf(stderr, "fifo_auto: request failed: %s\n", e.what());
        }
        if (!write_answer(answer, line))
            std::fprintf(stderr, "fifo_auto: cannot write answer to %s\n", answer);
        if (once) break;
    }
    cpd_index_free(ix);
    cpd_graph_free(dg);
    cpd_plan_free(plan);
    if (arena) cpd_device_arena_release(device);
    return 0;
}
