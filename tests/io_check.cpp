// Test harness (tests/test_io_cpu.py): one subcommand per entry point of
// csrc/cpd_io.hpp, compiled from the library's own cpd_io.cpp on the host (no
// HIP, no libcpd).  Readers print what they read as lines of decimal numbers
// (bulk arrays raw little-endian into a given output file); writers take
// their content from a small binary input file the test wrote.  An exception
// is one line: "ERR <code> <message>" for a cpd::Error, "ERR other <what()>"
// for anything else; the exit status is 0 either way.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "cpd_internal.hpp"
#include "cpd_io.hpp"

namespace io = cpd::io;

namespace {

struct Usage : std::runtime_error {
    Usage() : std::runtime_error("usage") {}
};

// A binary input file, consumed front to back.
struct In {
    std::vector<char> raw;
    size_t at = 0;
    explicit In(const std::string& path) {
        std::FILE* f = std::fopen(path.c_str(), "rb");
        if (!f) throw std::runtime_error("harness: cannot open " + path);
        char buf[1 << 16];
        size_t k;
        while ((k = std::fread(buf, 1, sizeof buf, f)) > 0) raw.insert(raw.end(), buf, buf + k);
        std::fclose(f);
    }
    template <class T>
    T one() {
        T v;
        take(&v, sizeof v);
        return v;
    }
    template <class T>
    std::vector<T> many(size_t count) {
        std::vector<T> v(count);
        take(v.data(), count * sizeof(T));
        return v;
    }
    void take(void* p, size_t bytes) {
        if (bytes > raw.size() - at) throw std::runtime_error("harness: input file too short");
        if (bytes) std::memcpy(p, raw.data() + at, bytes);
        at += bytes;
    }
};

// A raw output file of the bulk arrays.
struct Out {
    std::FILE* f;
    explicit Out(const std::string& path) : f(std::fopen(path.c_str(), "wb")) {
        if (!f) throw std::runtime_error("harness: cannot write " + path);
    }
    ~Out() { std::fclose(f); }
    template <class T>
    void put(const std::vector<T>& v) {
        if (!v.empty()) std::fwrite(v.data(), sizeof(T), v.size(), f);
    }
};

template <class T>
void print_row(const char* name, const std::vector<T>& v) {
    std::printf("%s", name);
    for (const T& x : v) std::printf(" %lld", (long long)x);
    std::printf("\n");
}

uint64_t u64_arg(const char* s) { return std::strtoull(s, nullptr, 0); }
uint32_t u32_arg(const char* s) { return (uint32_t)std::strtoull(s, nullptr, 0); }

// Tasks in a shuffled order, dealt to 4 threads; the first exception is rethrown.
void run_shuffled(std::vector<std::function<void()>> tasks) {
    std::mt19937 rng(12345);
    std::shuffle(tasks.begin(), tasks.end(), rng);
    std::mutex mu;
    std::string failed;
    int code = 0;
    bool is_cpd = false, any = false;
    std::vector<std::thread> th;
    for (size_t t = 0; t < 4; ++t)
        th.emplace_back([&, t] {
            for (size_t i = t; i < tasks.size(); i += 4) {
                try {
                    tasks[i]();
                } catch (const cpd::Error& e) {
                    std::lock_guard<std::mutex> lock(mu);
                    if (!any) failed = e.what(), code = e.code, is_cpd = true, any = true;
                } catch (const std::exception& e) {
                    std::lock_guard<std::mutex> lock(mu);
                    if (!any) failed = e.what(), any = true;
                }
            }
        });
    for (auto& x : th) x.join();
    if (any && is_cpd) throw cpd::Error(code, failed);
    if (any) throw std::runtime_error(failed);
}

// u32 n bid method key maxworker nrows | u64 fingerprint total | targets |
// offsets[nrows + 1] | runs[total]
io::CpdBucket bucket_input(const std::string& path) {
    In in(path);
    io::CpdBucket b;
    b.n = in.one<uint32_t>();
    b.bid = in.one<uint32_t>();
    b.method = in.one<uint32_t>();
    b.key = in.one<uint32_t>();
    b.maxworker = in.one<uint32_t>();
    const uint32_t nrows = in.one<uint32_t>();
    b.fingerprint = in.one<uint64_t>();
    const uint64_t total = in.one<uint64_t>();
    b.targets = in.many<uint32_t>(nrows);
    b.offsets = in.many<uint64_t>((size_t)nrows + 1);
    b.runs = in.many<uint32_t>(total);
    return b;
}

void print_bucket(const io::CpdBucket& b, const std::string& out) {
    std::printf("n %u nrows %zu bid %u method %u key %u maxworker %u total %llu fingerprint %llu runs %zu\n",
                b.n, b.targets.size(), b.bid, b.method, b.key, b.maxworker,
                (unsigned long long)b.offsets.back(), (unsigned long long)b.fingerprint, b.runs.size());
    Out o(out);
    o.put(b.targets);
    o.put(b.offsets);
    o.put(b.runs);
}

int run(int argc, char** argv) {
    if (argc < 2) throw Usage();
    const std::string cmd = argv[1];
    auto need = [&](int k) {
        if (argc < k) throw Usage();
    };
    if (cmd == "xy") {
        need(3);
        const io::XYGraph g = io::read_xy(argv[2]);
        std::printf("n %u m %u\n", g.n, g.m);
        print_row("row_ptr", g.row_ptr);
        print_row("dst", g.dst);
        print_row("w", g.w);
        print_row("x", g.x);
        print_row("y", g.y);
    } else if (cmd == "diff") {  // diff XY DIFF
        need(4);
        const io::XYGraph g = io::read_xy(argv[2]);
        print_row("w", io::read_diff(argv[3], g));
    } else if (cmd == "scen") {
        need(3);
        const io::Pairs q = io::read_scen(argv[2]);
        std::printf("%zu\n", q.size());
        for (auto& p : q) std::printf("%u %u\n", p.first, p.second);
    } else if (cmd == "bucket") {  // bucket PATH OUT
        need(4);
        print_bucket(io::read_bucket(argv[2]), argv[3]);
    } else if (cmd == "bucket-head") {  // bucket-head PATH OUT
        need(4);
        print_bucket(io::read_bucket_head(argv[2]), argv[3]);
    } else if (cmd == "bucket-runs") {  // bucket-runs PATH first count OUT
        need(6);
        const io::CpdBucket head = io::read_bucket_head(argv[2]);
        const uint64_t first = u64_arg(argv[3]), count = u64_arg(argv[4]);
        std::vector<uint32_t> runs(count);
        io::read_bucket_runs(argv[2], head, first, count, runs.data());
        Out(argv[5]).put(runs);
        std::printf("%llu\n", (unsigned long long)count);
    } else if (cmd == "bucket-format") {
        need(3);
        std::printf("%d\n", io::bucket_format(argv[2]));
    } else if (cmd == "move-head") {  // move-head PATH [noparts]
        need(3);
        const bool parts = !(argc > 3 && std::string(argv[3]) == "noparts");
        const io::MoveBucket b = io::read_move_bucket_head(argv[2], parts);
        std::printf("n %u nrows %zu bid %u method %u key %u maxworker %u words %u bits %u total_runs %llu "
                    "fingerprint %llu stripes %u stripe_rows %u rows_offset %llu head_bytes %llu\n",
                    b.n, b.targets.size(), b.bid, b.method, b.key, b.maxworker, b.words, b.bits,
                    (unsigned long long)b.total_runs, (unsigned long long)b.fingerprint, b.stripes,
                    b.stripe_rows, (unsigned long long)b.rows_offset(), (unsigned long long)b.head_bytes());
        print_row("targets", b.targets);
        print_row("counts", b.counts);
    } else if (cmd == "move-rows") {  // move-rows PATH first count threads OUT
        need(7);
        const io::MoveBucket head = io::read_move_bucket_head(argv[2]);
        const uint32_t first = u32_arg(argv[3]), count = u32_arg(argv[4]);
        std::vector<uint32_t> rows((size_t)count * head.words);
        io::read_move_bucket_rows(argv[2], head, first, count, rows.data(), std::atoi(argv[5]));
        Out(argv[6]).put(rows);
        std::printf("%u\n", count);
    } else if (cmd == "bucket-runs-windows") {  // every (first, count) window, back to back into OUT
        need(4);
        const io::CpdBucket head = io::read_bucket_head(argv[2]);
        const uint64_t total = head.offsets.back();
        Out o(argv[3]);
        for (uint64_t first = 0; first <= total; ++first)
            for (uint64_t count = 0; first + count <= total; ++count) {
                std::vector<uint32_t> runs(count, 0xDEADBEEFu);
                io::read_bucket_runs(argv[2], head, first, count, runs.data());
                o.put(runs);
            }
        std::printf("%llu\n", (unsigned long long)total);
    } else if (cmd == "move-rows-windows") {  // move-rows-windows PATH threads OUT: the same for rows
        need(5);
        const io::MoveBucket head = io::read_move_bucket_head(argv[2]);
        const uint32_t nrows = (uint32_t)head.targets.size();
        Out o(argv[4]);
        for (uint32_t first = 0; first <= nrows; ++first)
            for (uint32_t count = 0; first + count <= nrows; ++count) {
                std::vector<uint32_t> rows((size_t)count * head.words, 0xDEADBEEFu);
                io::read_move_bucket_rows(argv[2], head, first, count, rows.data(), std::atoi(argv[3]));
                o.put(rows);
            }
        std::printf("%u\n", nrows);
    } else if (cmd == "order") {  // order PATH fp
        need(4);
        const std::vector<uint32_t> order = io::read_order(argv[2], u64_arg(argv[3]));
        std::printf("%zu\n", order.size());
        print_row("order", order);
    } else if (cmd == "order-n") {
        need(3);
        std::printf("%u\n", io::read_order_n(argv[2]));
    } else if (cmd == "write-xy") {  // write-xy IN OUT [nocoords]
        need(4);
        In in(argv[2]);  // u32 n m | row_ptr[n + 1] | dst[m] | w[m] | i32 x[n] | y[n]
        const uint32_t n = in.one<uint32_t>(), m = in.one<uint32_t>();
        const auto row_ptr = in.many<uint32_t>((size_t)n + 1);
        const auto dst = in.many<uint32_t>(m), w = in.many<uint32_t>(m);
        const auto x = in.many<int32_t>(n), y = in.many<int32_t>(n);
        const bool coords = !(argc > 4 && std::string(argv[4]) == "nocoords");
        io::write_xy(argv[3], n, row_ptr.data(), dst.data(), w.data(), coords ? x.data() : nullptr,
                     coords ? y.data() : nullptr);
        std::printf("ok\n");
    } else if (cmd == "write-diff") {  // write-diff XY IN OUT
        need(5);
        const io::XYGraph g = io::read_xy(argv[2]);
        In in(argv[3]);  // u32 m | w[m]
        const uint32_t m = in.one<uint32_t>();
        if (m != g.m) throw std::runtime_error("harness: weight count != edge count");
        io::write_diff(argv[4], g, in.many<uint32_t>(m));
        std::printf("ok\n");
    } else if (cmd == "write-scen") {  // write-scen IN OUT
        need(4);
        In in(argv[2]);  // u32 count | (s, t)[count]
        const uint32_t count = in.one<uint32_t>();
        io::Pairs q(count);
        for (auto& p : q) {
            p.first = in.one<uint32_t>();
            p.second = in.one<uint32_t>();
        }
        io::write_scen(argv[3], q);
        std::printf("ok\n");
    } else if (cmd == "write-bucket") {  // write-bucket IN OUT
        need(4);
        io::write_bucket(argv[3], bucket_input(argv[2]));
        std::printf("ok\n");
    } else if (cmd == "bucket-pieces") {  // bucket-pieces IN OUT [noclose]
        need(4);
        const io::CpdBucket b = bucket_input(argv[2]);
        const bool close = !(argc > 4 && std::string(argv[4]) == "noclose");
        {
            io::BucketFile f(argv[3], b);
            std::vector<std::function<void()>> tasks;
            const uint32_t noff = (uint32_t)b.offsets.size();
            for (uint32_t r = 0; r < noff; r += 3)
                tasks.push_back([&, r] { f.write_offsets(r, b.offsets.data() + r, std::min(3u, noff - r)); });
            for (uint64_t r = 0; r < b.runs.size(); r += 5)
                tasks.push_back(
                    [&, r] { f.write_runs(r, b.runs.data() + r, std::min<uint64_t>(5, b.runs.size() - r)); });
            run_shuffled(tasks);
            if (close) f.close(b.offsets.back());
        }
        std::printf("ok\n");
    } else if (cmd == "move-pieces") {  // move-pieces IN OUT stripes stripe_rows [noclose]
        need(6);
        In in(argv[2]);  // u32 n bid method key maxworker words bits nrows | u64 fingerprint total |
                         // targets | counts | rows[nrows][words]
        io::MoveBucket b;
        b.n = in.one<uint32_t>();
        b.bid = in.one<uint32_t>();
        b.method = in.one<uint32_t>();
        b.key = in.one<uint32_t>();
        b.maxworker = in.one<uint32_t>();
        b.words = in.one<uint32_t>();
        b.bits = in.one<uint32_t>();
        const uint32_t nrows = in.one<uint32_t>();
        b.fingerprint = in.one<uint64_t>();
        const uint64_t total = in.one<uint64_t>();
        b.targets = in.many<uint32_t>(nrows);
        const auto counts = in.many<uint32_t>(nrows);
        const auto rows = in.many<uint32_t>((size_t)nrows * b.words);
        const bool close = !(argc > 6 && std::string(argv[6]) == "noclose");
        {
            io::MoveBucketFile f(argv[3], b, u32_arg(argv[4]), u32_arg(argv[5]));
            std::vector<std::function<void()>> tasks;
            const uint32_t words = b.words;
            for (uint32_t r = 0; r < nrows; r += 3)
                tasks.push_back([&, r] { f.write_counts(r, counts.data() + r, std::min(3u, nrows - r)); });
            for (uint32_t r = 0; r < nrows; r += 5)  // pieces that straddle stripe units
                tasks.push_back(
                    [&, r] { f.write_rows(r, rows.data() + (size_t)r * words, std::min(5u, nrows - r)); });
            run_shuffled(tasks);
            if (close) f.close(total);
        }
        std::printf("ok\n");
    } else if (cmd == "write-order") {  // write-order IN OUT fp
        need(5);
        In in(argv[2]);  // u32 n | order[n]
        const uint32_t n = in.one<uint32_t>();
        io::write_order(argv[3], u64_arg(argv[4]), in.many<uint32_t>(n));
        std::printf("ok\n");
    } else if (cmd == "part-rows") {  // part-rows nrows S K
        need(5);
        io::MoveBucket b;
        b.targets.resize(u32_arg(argv[2]));
        b.stripe_rows = u32_arg(argv[3]);
        b.stripes = u32_arg(argv[4]);
        std::vector<uint64_t> rows;
        for (uint32_t j = 0; j < b.stripes; ++j) rows.push_back(b.part_rows(j));
        print_row("part_rows", rows);
    } else if (cmd == "part-rows-grid") {  // the same for every nrows <= N, 1 <= S <= MS, 1 <= K <= MK
        need(5);
        const uint32_t N = u32_arg(argv[2]), MS = u32_arg(argv[3]), MK = u32_arg(argv[4]);
        for (uint32_t nr = 0; nr <= N; ++nr)
            for (uint32_t S = 1; S <= MS; ++S)
                for (uint32_t K = 1; K <= MK; ++K) {
                    io::MoveBucket b;
                    b.targets.resize(nr);
                    b.stripe_rows = S;
                    b.stripes = K;
                    std::printf("%u %u %u", nr, S, K);
                    for (uint32_t j = 0; j < K; ++j) std::printf(" %llu", (unsigned long long)b.part_rows(j));
                    std::printf("\n");
                }
    } else {
        throw Usage();
    }
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    try {
        return run(argc, argv);
    } catch (const Usage&) {
        std::fprintf(stderr, "usage: io_check <subcommand> <arguments> (see tests/io_check.cpp)\n");
        return 2;
    } catch (const cpd::Error& e) {
        std::printf("ERR %d %s\n", e.code, e.what());
    } catch (const std::exception& e) {
        std::printf("ERR other %s\n", e.what());
    }
    return 0;
}
