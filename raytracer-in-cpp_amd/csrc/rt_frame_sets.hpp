// rt_frame_sets.hpp -- the bookkeeping of the two frame working sets of a context (rt_capi.cpp; DESIGN.md §5, Frames in flight): which set a
// call gets, which events it waits for and records on which stream, and when a set is outstanding.  It decides; rt_capi.cpp only executes the
// steps it returns, in order.  Header-only and free of HIP -- streams and events are named, never held -- so that a host program can drive it
// under a sanitizer beside a happens-before model of the streams (tools/frame_sets_check.cpp).
//
// The protocol.  A context has two working sets (everything a frame's launches write and later launches of the same frame read), an internal
// stream per set, and per set the events body_done and set_free.
//   an overlapped frame on set s, caller's stream T:
//       internal[s]: wait set_free[s] ; the frame's launches up to the resolve ; record body_done[s]
//       T:           wait body_done[s] ; k_resolve ; record set_free[s]
//   any other use of set 0 on a stream T (a frame that is not overlapped, a graph replay, listed rays), once the context has overlapped:
//       T:           wait set_free[s] of every set with a record outstanding ; the work ; record set_free[0]
//   a host wait (synchronise, upload, growth, destroy): the set_free events with a record outstanding and both internal streams; nothing is
//       outstanding behind it.
// set_free[s] is only ever recorded behind a wait for the record before it (or behind a host wait), so its latest record is behind every
// earlier use of set s: one wait orders a new use after all of them.  body_done[s] is recorded and waited for inside one call and never
// outlives it.  Before the first overlapped frame nothing is waited for or recorded: a context that never overlaps pays nothing; the first
// overlapped frame waits on the host, once, for the context's earlier frames and for its caller's stream (the uses of set 0 before it left no
// record); work the caller put on yet another stream is the caller's to order, as it was.  On a capturing stream nothing is waited for or
// recorded: a capture behind overlapped frames is the caller's to put behind a synchronise.
#pragma once

#include <cstdint>

namespace rtamd {

enum class FsStream : uint8_t { CALLER, INTERNAL0, INTERNAL1 };
enum class FsEvent : uint8_t { BODY_DONE0, BODY_DONE1, SET_FREE0, SET_FREE1 };
inline FsStream fs_internal(const int set) { return set ? FsStream::INTERNAL1 : FsStream::INTERNAL0; }
inline FsEvent fs_body_done(const int set) { return set ? FsEvent::BODY_DONE1 : FsEvent::BODY_DONE0; }
inline FsEvent fs_set_free(const int set) { return set ? FsEvent::SET_FREE1 : FsEvent::SET_FREE0; }

struct FsStep {
    enum Op : uint8_t {
        WAIT,              // `stream` waits for `event`
        RECORD,            // `event` is recorded on `stream`
        BODY,              // the launches of the frame up to and excluding the resolve, on `stream` (an internal one), on set `set`
        RESOLVE,           // k_resolve of set `set` on `stream` (the caller's)
        HOST_WAIT_EVENT,   // the host waits for `event`
        HOST_WAIT_STREAM,  // the host waits for `stream` (an internal one)
        HOST_WAIT_FRAMES   // the host waits for the frames the context has enqueued so far (its own stream, the stream of its latest frame) and for
                           // the caller's stream of this call
    } op;
    FsStream stream;
    FsEvent event;
};
struct FsSteps {
    static constexpr int kMax = 8;
    FsStep step[kMax];
    int n = 0;
    int set = 0;           // the set of the call's own work
    void add(const FsStep::Op op, const FsStream st, const FsEvent ev) { step[n++] = FsStep{op, st, ev}; }
};

// what rt_render_device knows of a frame when it chooses the route
struct FsFrame {
    bool plain;            // FramePlan::PLAIN
    bool stats;            // the caller asked for rt_stats
    bool collect;          // collect_stats != 0
    bool hit_ids;          // d_out_hit != nullptr
    bool sphere_lights;    // the lights' offsets live in a buffer of the context that later calls rewrite
    bool capturing;        // the caller's stream is capturing
    bool idle;             // nothing to run beside: the caller's stream has drained and every outstanding set_free has completed (a lone frame
                           // takes the one-set route, which costs it no hop between streams; the frame behind it finds it in flight and overlaps)
};

class FrameSets {
public:
    // rt_set_frame_overlap
    void set_on(const bool v, const bool always = false) { on_ = v; always_ = v && always; }
    bool always() const { return always_; }      // a frame with nothing in flight to run beside overlaps too
    bool on() const { return on_; }
    // the second set and the internal streams exist
    bool ready() const { return ready_; }
    // the second set did not fit beside the first: this context takes the one-set route from now on
    void refuse() { refused_ = true; ready_ = false; }
    bool refused() const { return refused_; }
    // a set_free record of set s is outstanding (no host wait since)
    bool outstanding(const int s) const { return free_rec_[s]; }

    // Which frames take the overlapped route.
    bool admits(const FsFrame &f) const {
        return on_ && !refused_ && f.plain && !f.stats && !f.collect && !f.hit_ids && !f.sphere_lights && !f.capturing && (!f.idle || always_);
    }

    // The first overlapped frame, in front of overlapped_frame() and after the second set and the streams were made.
    FsSteps first_overlap() {
        FsSteps q;
        if (ready_) return q;
        q.add(FsStep::HOST_WAIT_FRAMES, FsStream::CALLER, FsEvent::SET_FREE0);
        ready_ = true;
        free_rec_[0] = free_rec_[1] = false;
        next_ = 0;
        return q;
    }

    // An overlapped frame: it takes the set the one before it did not take.
    FsSteps overlapped_frame() {
        FsSteps q;
        const int s = next_;
        next_ ^= 1;
        q.set = s;
        if (free_rec_[s]) q.add(FsStep::WAIT, fs_internal(s), fs_set_free(s));
        q.add(FsStep::BODY, fs_internal(s), fs_body_done(s));
        q.add(FsStep::RECORD, fs_internal(s), fs_body_done(s));
        q.add(FsStep::WAIT, FsStream::CALLER, fs_body_done(s));
        q.add(FsStep::RESOLVE, FsStream::CALLER, fs_set_free(s));
        q.add(FsStep::RECORD, FsStream::CALLER, fs_set_free(s));
        free_rec_[s] = true;
        return q;
    }

    // Any other use of set 0 on a stream: the drain in front of the work ...
    FsSteps before_set0_use(const bool capturing = false) const {
        FsSteps q;
        if (!ready_ || capturing) return q;
        for (int s = 0; s < 2; ++s)
            if (free_rec_[s]) q.add(FsStep::WAIT, FsStream::CALLER, fs_set_free(s));
        return q;
    }
    // ... and the record behind it.
    FsSteps after_set0_use(const bool capturing = false) {
        FsSteps q;
        if (!ready_ || capturing) return q;
        q.add(FsStep::RECORD, FsStream::CALLER, fs_set_free(0));
        free_rec_[0] = true;
        return q;
    }

    // A host wait for everything the protocol has in flight (the caller of this adds the context's own stream and the stream of its latest
    // frame, as before).  Nothing is outstanding behind it.
    FsSteps host_wait() {
        FsSteps q;
        if (!ready_) return q;
        for (int s = 0; s < 2; ++s)
            if (free_rec_[s]) q.add(FsStep::HOST_WAIT_EVENT, FsStream::CALLER, fs_set_free(s));
        q.add(FsStep::HOST_WAIT_STREAM, FsStream::INTERNAL0, FsEvent::SET_FREE0);
        q.add(FsStep::HOST_WAIT_STREAM, FsStream::INTERNAL1, FsEvent::SET_FREE1);
        free_rec_[0] = free_rec_[1] = false;
        return q;
    }

private:
    bool on_ = true, always_ = false, ready_ = false, refused_ = false;
    int next_ = 0;
    bool free_rec_[2] = {false, false};
};

}  // namespace rtamd
