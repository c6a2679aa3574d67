// Drives csrc/tail_wait.hpp alone, without a device: the comparison of the done / gave-up words with the armed generation, the
// bookkeeping "the tail launch and its fallback are the last thing enqueued on the main stream", and the bounded poll (with a clock of
// its own, so that no real time has to pass).  Plain C++:
//   g++ -std=c++17 -Wall -Werror -o tail_wait_check tail_wait_check.cpp && ./tail_wait_check        (-fsanitize=address,undefined works as well)
// Prints "tail_wait_check ok" and exits 0, or says which expectation failed and exits 1.
#include "../csrc/tail_wait.hpp"

#include <cstdio>
#include <cstdlib>

static int failures = 0;
#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); failures++; } \
    } while (0)

int main() {
    // ---- the comparison -------------------------------------------------------------------------------------------
    EXPECT(!TailWait::complete(0, 0, 0));                  // nothing armed (generations skip 0; the words start at 0)
    EXPECT(!TailWait::complete(0, 0, 1));                  // the context's first launch, still running
    EXPECT(TailWait::complete(1, 0, 1));                   // ... done
    EXPECT(!TailWait::complete(1, 1, 1));                  // ... done, but a group gave up: the fallback is at work
    EXPECT(TailWait::complete(7, 6, 7));                   // an OLDER launch gave up: not this one's business
    EXPECT(!TailWait::complete(6, 0, 7));                  // the previous launch's word
    EXPECT(!TailWait::complete(8, 0, 7));                  // (cannot happen: the armed launch is the last enqueued) — not equal, not complete
    EXPECT(TailWait::complete(0xffffffffu, 5, 0xffffffffu));          // the last generation before the counter comes round
    EXPECT(!TailWait::complete(0xffffffffu, 0, 1));                   // ... and the first one after it, still running
    EXPECT(TailWait::complete(1, 0xffffffffu, 1));                    // ... done; the give-up of 2^32 - 1 launches ago is not its own

    // ---- the bookkeeping --------------------------------------------------------------------------------------------
    unsigned words[32] = {0};
    TailWait t;
    t.done = words; t.gave_up = words + 16;
    long long now = 0;
    int ticks = 0;
    auto clock = [&] { ticks++; return now += 10; };      // every look at the clock: 10 us later
    EXPECT(!t.poll(clock));                                // nothing armed: the caller waits for the stream
    t.note_top(3);
    EXPECT(t.armed == 0);                                  // noted, not armed: the caller may still enqueue (a download's export kernel)
    t.arm();
    EXPECT(t.armed == 3 && t.top == 0);
    t.enqueued();                                          // something else goes onto the stream
    EXPECT(t.armed == 0 && !t.poll(clock));
    t.note_top(4); t.enqueued(); t.arm();                  // an enqueue between the note and the arming voids the note
    EXPECT(t.armed == 0);
    t.note_top(0); t.arm();                                // read_top's last launch was not the tail
    EXPECT(t.armed == 0);
    t.note_top(5); t.arm(); t.waited();                    // the host waited for the stream
    EXPECT(t.armed == 0);

    // ---- the poll -----------------------------------------------------------------------------------------------------
    t.note_top(9); t.arm();
    words[0] = 9;
    ticks = 0;
    EXPECT(t.poll(clock) && ticks == 0);                   // done at the first look: the clock is not even read
    words[0] = 8;
    t.bound_us = 300; ticks = 0;
    EXPECT(!t.poll(clock));                                // never done: the bound runs out
    EXPECT(ticks >= 30 && ticks <= 32);                    // ... after 300 us of the clock above, not before, not long after
    t.bound_us = 0; ticks = 0;
    EXPECT(!t.poll(clock) && ticks == 0);                  // bound 0: one look
    words[0] = 9;
    EXPECT(t.poll(clock));                                 // ... which is enough for a host that comes late
    t.bound_us = -1;
    EXPECT(!t.poll(clock));                                // never look
    t.bound_us = 300;
    words[16] = 9; ticks = 0;
    EXPECT(!t.poll(clock) && ticks <= 1);                  // gave up: straight to the stream wait, no spinning
    // the word arrives while the host polls
    words[0] = 8; words[16] = 0;
    int looks = 0;
    auto clock2 = [&] { if (++looks == 5) words[0] = 9; return now += 10; };
    EXPECT(t.poll(clock2) && looks >= 5 && looks <= 6);
    EXPECT(t.armed == 9);                                  // polling changes nothing: fheram_sync's main_waited() disarms
    // the real clock: a bound that cannot be met ends the poll (a few hundred microseconds of wall time)
    words[0] = 8; t.bound_us = 200;
    EXPECT(!t.poll());

    if (failures) return 1;
    std::printf("tail_wait_check ok\n");
    return 0;
}
