// The sampler's step-count read-ahead (glmmrmcml_amd/csrc/step_ahead.h) against a simulated device and clock, as plain
// C++ under AddressSanitizer + UBSan.  The "device" is a queue of (sequence number, count) tokens that reach the ring of
// StepAhead::SLOTS slots when the simulation says so: at once, one per reading of the clock (a GPU that lags behind the
// host), or never.  A synchronisation delivers everything that is queued, as hipStreamSynchronize does.  Every scenario
// prints "scenario NAME fails=K"; built and run by tests/test_step_ahead_cpu.py.
#include "step_ahead.h"
#include <cstdio>
#include <deque>
#include <utility>
using namespace mcml;

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { printf("  line %d: ", __LINE__); printf(__VA_ARGS__); printf("\n"); ++fails; } } while (0)

// the figures are written out here, not taken from the header: 8 slots, 8 counts at the cap before the first speculation,
// at most 4 unobserved proposals, 2000 ms
constexpr int CAP = 10, SLOTS = 8, STREAK = 8, AHEAD = 4, SYNC = StepAhead::SYNCHRONISE;
constexpr double GIVE_UP_MS = 2000.0;
static_assert(StepAhead::SLOTS == SLOTS, "the ring of ctx.h has StepAhead::SLOTS slots");

struct Sim {
    unsigned long long ring[SLOTS] = {};
    unsigned seq = 0;                                   // StepRing::seq: the last proposal launched, over all calls
    std::deque<std::pair<unsigned, int>> queued;        // launched, count not yet in the ring
    double now = 0, tick = 0.001;                       // simulated clock (ms) and what one reading of it costs
    int per_tick = 0, tick_div = 1;                     // per_tick tokens arrive with every tick_div-th reading of the clock
    long clock_reads = 0;

    static unsigned long long token(unsigned sq, int count) { return ((unsigned long long)sq << 32) | (unsigned)count; }
    void deliver(int k) { for (; k > 0 && !queued.empty(); --k) { ring[queued.front().first % SLOTS] = token(queued.front().first, queued.front().second); queued.pop_front(); } }
    void deliver_all() { deliver((int)queued.size()); }
    unsigned launch(int count) { queued.emplace_back(++seq, count); return seq; }
    auto clock() { return [this] { now += tick; if (++clock_reads % tick_div == 0) deliver(per_tick); return now; }; }
    // one proposal as hmc_sample runs it: -> the number of steps launched; *synced: it waited for the device
    int propose(StepAhead& a, int count, bool* synced)
    {
        const unsigned sq = launch(count);
        int maxs = a.launched(sq, clock());
        *synced = maxs == SYNC;
        if (*synced) { deliver_all(); maxs = a.synchronised(sq); }
        return maxs;
    }
};

static void finish(const char* name) { printf("scenario %s fails=%d\n", name, fails); fails = 0; }

// 1. every count at the cap: the first SPEC_STREAK proposals synchronise, then the cap is launched without waiting
static void scenario_warm_up()
{
    Sim s; StepAhead a(s.ring, s.seq, CAP, true);
    for (int i = 1; i <= 40; ++i) {
        bool synced;
        const int streak_before = a.streak;
        const int maxs = s.propose(a, CAP, &synced);
        CHECK(maxs == CAP, "proposal %d: %d steps", i, maxs);
        CHECK(synced == (i <= 8), "proposal %d: synced %d", i, (int)synced);
        CHECK(synced || streak_before >= 8, "proposal %d speculated on a streak of %d", i, streak_before);
        if (!synced) s.deliver_all();                   // the count arrives before the next proposal
    }
    // the same with the speculation switched off (GLMMR_MCML_HMC_SPEC=0): always the exact path
    Sim s0; StepAhead a0(s0.ring, s0.seq, CAP, false);
    for (int i = 1; i <= 20; ++i) {
        bool synced;
        const int maxs = s0.propose(a0, CAP, &synced);
        CHECK(synced && maxs == CAP, "not allowed, proposal %d: synced %d, %d steps", i, (int)synced, maxs);
    }
    finish("warm_up");
}

// 2. one count of 9 ends the speculation at the next decision; it resumes after 8 more at the cap, not before
static void scenario_below_cap()
{
    Sim s; StepAhead a(s.ring, s.seq, CAP, true);
    bool synced;
    for (int i = 1; i <= 12; ++i) { s.propose(a, CAP, &synced); if (!synced) s.deliver_all(); }
    CHECK(!synced, "speculating before the low count");
    int maxs = s.propose(a, 9, &synced);                // its count is not known when it is decided
    CHECK(!synced && maxs == CAP, "the proposal whose count is 9: synced %d, %d steps", (int)synced, maxs);
    s.deliver_all();
    int nsync = 0;
    for (int i = 1; i <= 20; ++i) {
        maxs = s.propose(a, CAP, &synced);
        CHECK(maxs == CAP, "after the low count, proposal %d: %d steps", i, maxs);
        CHECK(synced == (i <= 8), "after the low count, proposal %d: synced %d", i, (int)synced);
        nsync += synced;
        if (!synced) s.deliver_all();
    }
    CHECK(nsync == 8, "%d synchronous proposals after the low count", nsync);
    // a count below the cap on the synchronous path is returned as it is and keeps the streak at zero
    maxs = s.propose(a, CAP, &synced); s.deliver_all();
    maxs = s.propose(a, 3, &synced); s.deliver_all();   // decided while speculating: the cap
    maxs = s.propose(a, 7, &synced);
    CHECK(synced && maxs == 7 && a.streak == 0, "synchronous low count: synced %d, %d steps, streak %d", (int)synced, maxs, a.streak);
    finish("below_cap");
}

// 3. never more than AHEAD unobserved proposals behind a speculative decision; a count that does not come: synchronise
static void scenario_look_ahead()
{
    Sim s; StepAhead a(s.ring, s.seq, CAP, true);
    bool synced;
    for (int i = 1; i <= 8; ++i) s.propose(a, CAP, &synced);
    s.per_tick = 1; s.tick_div = 3;                     // a device that lags: a count per three readings of the clock, none otherwise
    const long reads0 = s.clock_reads;
    for (int i = 1; i <= 60; ++i) {
        const unsigned sq = s.launch(CAP);
        const int maxs = a.launched(sq, s.clock());
        CHECK(maxs == CAP, "lagging device, proposal %d: %d", i, maxs);
        CHECK((int)(sq - a.seen_seq) <= AHEAD, "proposal %d decided with %d counts outstanding", i, (int)(sq - a.seen_seq));
    }
    CHECK(s.clock_reads - reads0 >= 2 * 60, "the host did wait for the lagging device: %ld readings of the clock", s.clock_reads - reads0);
    // ... and a low count is noticed within AHEAD proposals of its launch
    const unsigned low = s.launch(9);
    int maxs = a.launched(low, s.clock());
    int n_after = 0;
    while (maxs != SYNC && n_after < 20) { ++n_after; maxs = a.launched(s.launch(CAP), s.clock()); }
    CHECK(n_after >= 1 && n_after <= AHEAD, "low count noticed after %d further proposals", n_after);
    s.deliver_all();
    CHECK(a.synchronised(s.seq) == CAP, "synchronise after the low count");
    // arrivals withheld: the look-ahead gives up once the clock has passed GIVE_UP_MS and asks for a synchronisation
    s.per_tick = 0; s.tick_div = 1;
    for (int i = 1; i <= 12; ++i) { s.propose(a, CAP, &synced); if (!synced) s.deliver_all(); }
    a.harvest();
    CHECK(!synced && a.streak >= STREAK && a.seen_seq == s.seq, "speculating again: streak %d", a.streak);
    s.tick = 100.0;
    for (int i = 1; i <= AHEAD; ++i) {
        const long r0 = s.clock_reads;
        maxs = a.launched(s.launch(CAP), s.clock());
        CHECK(maxs == CAP && s.clock_reads == r0 + 1, "withheld, proposal %d: %d steps, %ld readings of the clock", i, maxs, s.clock_reads - r0);   // within AHEAD: no waiting
    }
    const double t0 = s.now;
    const unsigned sq = s.launch(CAP);
    maxs = a.launched(sq, s.clock());
    CHECK(maxs == SYNC, "withheld, proposal %d: %d", AHEAD + 1, maxs);
    CHECK(s.now - t0 > GIVE_UP_MS && s.now - t0 <= GIVE_UP_MS + 3 * s.tick, "gave up after %.0f ms", s.now - t0);
    CHECK((int)(sq - a.seen_seq) == AHEAD + 1, "outstanding %d", (int)(sq - a.seen_seq));
    s.deliver_all();
    CHECK(a.synchronised(sq) == CAP && a.seen_seq == sq, "synchronise after giving up");
    finish("look_ahead");
}

// 4. a slot that carries another proposal's sequence number: not arrived for harvest, an error after a synchronisation
static void scenario_foreign_token()
{
    Sim s; StepAhead a(s.ring, s.seq, CAP, true);
    bool synced;
    for (int i = 1; i <= 3; ++i) s.propose(a, CAP, &synced);
    unsigned sq = s.launch(CAP);                        // proposal 4, its slot holds the token of a proposal SLOTS later / earlier
    for (unsigned other : {sq + SLOTS, sq - SLOTS, 0u}) {
        s.ring[sq % SLOTS] = Sim::token(other, CAP);
        a.last_seq = sq;
        CHECK(a.harvest() == 0 && a.seen_seq == sq - 1, "foreign token %u harvested", other);
        CHECK(a.launched(sq, s.clock()) == SYNC, "foreign token %u: decision", other);
        CHECK(a.synchronised(sq) == StepAhead::NOT_ARRIVED, "foreign token %u after a synchronisation", other);
        CHECK(a.seen_seq == sq - 1 && a.streak == 3, "foreign token %u changed the state", other);
    }
    s.queued.clear();
    s.ring[sq % SLOTS] = Sim::token(sq, CAP);
    CHECK(a.synchronised(sq) == CAP, "the right token");
    // proposal 6 is there, proposal 5 is not: the counts are observed in order or not at all
    s.launch(CAP); sq = s.launch(CAP); s.queued.clear();
    s.ring[sq % SLOTS] = Sim::token(sq, CAP);
    a.last_seq = sq;
    CHECK(a.harvest() == 0, "harvest past a missing count");
    CHECK(a.synchronised(sq) == StepAhead::OUT_OF_ORDER, "a missing count before the one waited for");
    finish("foreign_token");
}

// 5. two calls share one ring: the sequence numbers go on, every call gathers its own evidence
static void scenario_two_calls()
{
    Sim s;
    bool synced;
    {
        StepAhead a(s.ring, s.seq, CAP, true);
        for (int i = 1; i <= 11; ++i) { s.propose(a, CAP, &synced); if (!synced) s.deliver_all(); }
        a.harvest();
        CHECK(s.seq == 11 && a.seen_seq == 11 && !synced, "first call: seq %u seen %u", s.seq, a.seen_seq);
    }
    StepAhead b(s.ring, s.seq, CAP, true);
    CHECK(b.seen_seq == 11 && b.last_seq == 11 && b.streak == 0 && b.seen_maxs == -1, "second call starts from the counter");
    CHECK(b.harvest() == 0, "the first call's tokens are not the second call's");
    for (int i = 1; i <= 12; ++i) {
        const int maxs = s.propose(b, i == 2 ? 6 : CAP, &synced);
        CHECK(s.seq == 11u + i && (!synced || (s.ring[s.seq % SLOTS] >> 32) == s.seq), "second call, proposal %d: slot", i);
        CHECK(maxs == (i == 2 ? 6 : CAP), "second call, proposal %d: %d steps", i, maxs);
        CHECK(synced == (i <= 10), "second call, proposal %d: synced %d", i, (int)synced);      // 2 + 8 at the cap
        if (!synced) s.deliver_all();
    }
    // the counter wraps like any unsigned
    Sim w; w.seq = 0xfffffffcu;
    for (unsigned sq = w.seq - (SLOTS - 1); sq != w.seq + 1; ++sq) w.ring[sq % SLOTS] = Sim::token(sq, CAP);   // what earlier proposals left
    StepAhead c(w.ring, w.seq, CAP, true);
    for (int i = 1; i <= 12; ++i) {
        const int maxs = w.propose(c, CAP, &synced);
        CHECK(maxs == CAP && synced == (i <= 8), "across the wrap, proposal %d: %d steps, synced %d", i, maxs, (int)synced);
        if (!synced) w.deliver_all();
    }
    CHECK(w.seq == 8u, "wrapped counter %u", w.seq);
    finish("two_calls");
}

int main()
{
    scenario_warm_up();
    scenario_below_cap();
    scenario_look_ahead();
    scenario_foreign_token();
    scenario_two_calls();
    return 0;
}
