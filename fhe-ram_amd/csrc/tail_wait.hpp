// The host's short cut at the end of a read-type operation (plain C++: no HIP call in here; host/tail_wait_check.cpp drives it alone).
//
// A read or read_prepare_write ends with k_trace_tail and, behind it, the predicated fallback launch that only works if the tail gave up.
// That launch starts, finds its predicate false and ends: 4-5 us of launch and end-of-kernel processing the host used to wait for.  The
// tail's last workgroup to leave writes the launch's generation into a host-mapped word (`done`), a workgroup whose group gave up writes
// it into a second one (`gave_up`) before it is counted as gone.  done == seq and gave_up != seq: every store of the operation has been
// performed and the launch behind it will write nothing — the operation is complete for the host.  Anything else: wait for the stream.
//
// Which generation to look for is bookkeeping on the enqueue side:
//   note_top(seq)  read_top's last launch pair was the tail of generation seq and its fallback (0: it was something else)
//   arm()          the operation that called read_top has enqueued nothing behind it (fheram_read / fheram_read_prepare_write without a download)
//   enqueued()     something with an effect on memory goes onto the main stream (ctx.hpp main_enqueued); waited(): the host has waited for it
// so armed != 0 exactly while that launch pair is the last thing enqueued on the main stream.
#pragma once
#include <chrono>

struct TailWait {
    const volatile unsigned* done = nullptr;      // host-mapped, written by the device: generation of the last tail launch whose workgroups have all left
    const volatile unsigned* gave_up = nullptr;   // ... of the last tail launch in which a group gave up
    unsigned top = 0, armed = 0;
    long bound_us = 2000;   // the poll's bound in host time; 0: one look; < 0: never look (FHERAM_TAIL_POLL_US).  A read-type operation at the
                            // largest size whose chains are one workgroup round takes 0.5 ms; past the bound the runtime's own wait takes over
    void note_top(unsigned seq) { top = seq; }
    void arm() { armed = top; top = 0; }
    void enqueued() { top = armed = 0; }
    void waited() { top = armed = 0; }

    // The comparison is for EQUALITY with the armed generation: launches of one stream complete in order and the armed one is the last
    // enqueued, so `done` can only hold an older generation or this one (generations skip 0 and come round after 2^32 launches).
    static bool complete(unsigned done_word, unsigned gave_up_word, unsigned seq) { return seq != 0 && done_word == seq && gave_up_word != seq; }

    // one look at the words: `done` first — the device writes gave_up, then (behind a fence) done
    bool look() const {
        if (!armed || !done || !gave_up) return false;
        const unsigned d = __atomic_load_n(const_cast<const unsigned*>(done), __ATOMIC_ACQUIRE);
        const unsigned g = __atomic_load_n(const_cast<const unsigned*>(gave_up), __ATOMIC_ACQUIRE);
        return complete(d, g, armed);
    }
    // true: the armed operation is complete; false: the caller waits for the stream as it always did (nothing armed, a group gave up, the
    // bound ran out).  now_us: a monotonic clock in microseconds (a parameter so that the check program can make time pass as it likes).
    template <typename Clock>
    bool poll(Clock&& now_us) const {
        if (!armed || bound_us < 0) return false;
        if (look()) return true;
        if (bound_us == 0) return false;
        const long long t0 = now_us();
        do {
            if (__atomic_load_n(const_cast<const unsigned*>(gave_up), __ATOMIC_RELAXED) == armed) return false;   // the fallback is at work: no point in spinning
            if (look()) return true;
        } while (now_us() - t0 < bound_us);
        return false;
    }
    bool poll() const {
        return poll([] { return (long long)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now().time_since_epoch()).count(); });
    }
};
