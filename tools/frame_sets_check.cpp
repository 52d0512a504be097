// Stand-alone host check of rt_frame_sets.hpp (the bookkeeping of the two frame working sets), meant for a sanitizer build on the CPU:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iraytracer-in-cpp_amd/csrc tools/frame_sets_check.cpp -o frame_sets_check
// (make -C raytracer-in-cpp_amd/csrc frame_sets_check builds and runs it).  Exit status 0: every check held.
//
// It drives the unit with long pseudo-random sequences of every call kind on up to three caller streams -- overlapped frame, frame on the
// one-set route, graph launch, query, upload, synchronise, the switch -- and executes the steps the unit returns on a happens-before model
// of streams and events: every operation has a number; a stream, an event and the host each hold the set of operations known to be complete
// before whatever comes next on them.  The invariant: any two operations that touch the same working set are ordered, and every k_resolve is
// on its caller's stream (so behind the caller's earlier work there) and behind its own body.  Two uses of set 0 that BOTH took the one-set
// route before the context ever overlapped are the caller's to order, as they always were, and are not judged.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "rt_frame_sets.hpp"

using namespace rtamd;

static int failures = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

using OpSet = std::vector<bool>;       // indexed by operation number
static void merge(OpSet &into, const OpSet &from) {
    if (into.size() < from.size()) into.resize(from.size(), false);
    for (size_t i = 0; i < from.size(); ++i)
        if (from[i]) into[i] = true;
}
static bool has(const OpSet &s, const size_t i) { return i < s.size() && s[i]; }

struct Op {
    int touches;          // bit s: it reads or writes set s
    bool judged;          // (see above: uses of set 0 before the context ever overlapped are not)
};

struct Model {
    static constexpr int kCallers = 3;
    OpSet stream[kCallers + 2];     // the caller's streams, then the two internal ones
    OpSet event[4];
    OpSet host;
    std::vector<Op> ops;
    int caller = 0;                 // the caller's stream of the call being executed

    OpSet &of(const FsStream s) { return s == FsStream::CALLER ? stream[caller] : stream[kCallers + (s == FsStream::INTERNAL1 ? 1 : 0)]; }

    // an operation enqueued on `st`: behind what the stream holds and what the host has waited for
    size_t enqueue(OpSet &st, const int touches, const bool judged) {
        merge(st, host);
        const size_t id = ops.size();
        for (size_t k = 0; k < id; ++k)
            if ((ops[k].touches & touches) != 0 && (ops[k].judged || judged)) CHECK(has(st, k));
        ops.push_back(Op{touches, judged});
        if (st.size() <= id) st.resize(id + 1, false);
        st[id] = true;
        return id;
    }
    // an operation of the host itself (a copy into the buffers, their reallocation): behind everything it has waited for
    void host_op(const int touches) {
        for (size_t k = 0; k < ops.size(); ++k)
            if ((ops[k].touches & touches) != 0 && ops[k].judged) CHECK(has(host, k));
    }
    void host_waits_all() { host.assign(ops.size(), true); }

    // executes what the unit returned
    void run(const FsSteps &q) {
        size_t body = SIZE_MAX;
        for (int i = 0; i < q.n; ++i) {
            const FsStep &s = q.step[i];
            switch (s.op) {
            case FsStep::WAIT: merge(of(s.stream), event[static_cast<int>(s.event)]); break;
            case FsStep::RECORD: merge(of(s.stream), host); event[static_cast<int>(s.event)] = of(s.stream); break;
            case FsStep::BODY:
                CHECK(s.stream == fs_internal(q.set));
                body = enqueue(of(s.stream), 1 << q.set, true);
                break;
            case FsStep::RESOLVE: {
                CHECK(s.stream == FsStream::CALLER);          // on the caller's stream: behind the caller's earlier work, in call order
                CHECK(body != SIZE_MAX);
                const size_t r = enqueue(of(s.stream), 1 << q.set, true);
                CHECK(has(of(s.stream), body) && r > body);
                break;
            }
            case FsStep::HOST_WAIT_EVENT: merge(host, event[static_cast<int>(s.event)]); break;
            case FsStep::HOST_WAIT_STREAM: merge(host, of(s.stream)); break;
            case FsStep::HOST_WAIT_FRAMES: host_waits_all(); break;      // (the model's callers order their other streams themselves: see above)
            }
        }
    }
};

static uint32_t rng_state = 1;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

static void sequence(const uint32_t seed, const int calls, const int callers) {
    rng_state = seed;
    FrameSets fs;
    Model m;
    int last_set = -1;
    for (int k = 0; k < calls; ++k) {
        m.caller = static_cast<int>(rnd() % static_cast<uint32_t>(callers));
        const uint32_t kind = rnd() % 16;
        if (kind < 8) {
            // a frame: the unit's rule decides the route (an eighth of them is something the rule refuses)
            const uint32_t odd = rnd() % 48;
            const FsFrame f{odd != 0, odd == 1, odd == 2, odd == 3, odd == 4, odd == 5, odd == 6 || odd == 7};
            const bool expect = fs.on() && !fs.refused() && (odd > 7 || (fs.always() && odd > 5));
            CHECK(fs.admits(f) == expect);
            if (fs.admits(f)) {
                if (!fs.ready()) { m.run(fs.first_overlap()); CHECK(fs.ready()); }
                const FsSteps q = fs.overlapped_frame();
                CHECK(q.n <= FsSteps::kMax && (q.set == 0 || q.set == 1));
                CHECK(last_set < 0 || q.set != last_set);        // the set the overlapped frame before it did not use
                last_set = q.set;
                m.run(q);
                CHECK(fs.outstanding(q.set));
                continue;
            }
        }
        if (kind < 13) {
            // a use of set 0 on the caller's stream: a frame on the one-set route, a graph launch, a query
            m.run(fs.before_set0_use());
            m.enqueue(m.of(FsStream::CALLER), 1, fs.ready());
            const FsSteps a = fs.after_set0_use();
            CHECK(a.n == (fs.ready() ? 1 : 0));
            m.run(a);
        } else if (kind == 13) {
            // synchronise, or the wait in front of an upload or of growth: the host then touches both sets.  (Before the context overlapped the
            // host waits for the streams it always waited for; the model lets it wait for all of them.)
            if (!fs.ready()) m.host_waits_all();
            m.run(fs.host_wait());
            m.host_op(3);
            CHECK(!fs.outstanding(0) && !fs.outstanding(1));
        } else if (kind == 14) {
            fs.set_on(rnd() % 2 != 0, rnd() % 4 == 0);
        } else if (rnd() % 64 == 0) {
            // the second set no longer fits: after a wait for everything, the one-set route for good
            if (!fs.ready()) m.host_waits_all();
            m.run(fs.host_wait());
            m.host_op(3);
            fs.refuse();
            CHECK(!fs.ready() && fs.refused());
        }
    }
}

int main() {
    // the rule, case by case
    {
        FrameSets fs;
        const FsFrame ok{true, false, false, false, false, false, false};
        CHECK(fs.on() && fs.admits(ok) && !fs.ready());
        FsFrame f = ok; f.plain = false; CHECK(!fs.admits(f));
        f = ok; f.stats = true; CHECK(!fs.admits(f));
        f = ok; f.collect = true; CHECK(!fs.admits(f));
        f = ok; f.hit_ids = true; CHECK(!fs.admits(f));
        f = ok; f.sphere_lights = true; CHECK(!fs.admits(f));
        f = ok; f.capturing = true; CHECK(!fs.admits(f));
        f = ok; f.idle = true; CHECK(!fs.admits(f));
        fs.set_on(true, true); CHECK(fs.admits(f) && fs.always()); fs.set_on(false, true); CHECK(!fs.admits(f) && !fs.always());
        fs.set_on(false); CHECK(!fs.admits(ok));
        fs.set_on(true); CHECK(fs.admits(ok));
        // a context that never overlaps pays nothing
        CHECK(fs.before_set0_use().n == 0 && fs.after_set0_use().n == 0 && fs.host_wait().n == 0);
        // the first frames: device wait once, sets 0, 1, 0; the third waits for the first's set_free, the second for nothing
        CHECK(fs.first_overlap().n == 1 && fs.first_overlap().n == 0);
        FsSteps a = fs.overlapped_frame(), b = fs.overlapped_frame(), c = fs.overlapped_frame();
        CHECK(a.set == 0 && b.set == 1 && c.set == 0 && a.n == 5 && b.n == 5 && c.n == 6);
        CHECK(c.step[0].op == FsStep::WAIT && c.step[0].stream == FsStream::INTERNAL0 && c.step[0].event == FsEvent::SET_FREE0);
        CHECK(c.step[4].op == FsStep::RESOLVE && c.step[4].stream == FsStream::CALLER && c.step[5].op == FsStep::RECORD && c.step[5].event == FsEvent::SET_FREE0);
        // the drain waits for both sets, the record is set 0's; a host wait leaves nothing outstanding
        CHECK(fs.before_set0_use(true).n == 0 && fs.after_set0_use(true).n == 0);      // (a capturing stream: neither)
        CHECK(fs.before_set0_use().n == 2 && fs.after_set0_use().n == 1);
        CHECK(fs.host_wait().n == 4 && !fs.outstanding(0) && !fs.outstanding(1) && fs.before_set0_use().n == 0 && fs.host_wait().n == 2);
        fs.refuse();
        CHECK(!fs.admits(ok) && fs.before_set0_use().n == 0 && fs.after_set0_use().n == 0);
    }
    for (uint32_t seed = 1; seed <= 60; ++seed) sequence(seed, 1500, 1 + static_cast<int>(seed % 3));
    sequence(4242, 6000, 3);

    std::printf(failures ? "frame_sets_check: %d FAILED\n" : "frame_sets_check: all checks held\n", failures);
    return failures ? 1 : 0;
}
