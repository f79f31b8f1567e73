// step_ahead.h -- how many leapfrog iterations hmc_sample (hmc.hip) launches for a proposal without waiting for the device.
// Host only: no HIP call, so that tests/host_step_ahead_driver.cpp can run it against a simulated ring and clock.
//
// The number of leapfrog iterations to launch is the largest step count over the chains, a device value.  Reading it
// back costs a host synchronisation per proposal (~50 us of idle GPU).  While the step counts observed so far sit at
// the cap (lambda / e >= max_steps, the usual regime), the cap itself is launched without waiting -- iterations beyond
// a chain's own count are masked no-ops, so results are identical -- and the true value comes back on its own:
// k_max_steps stores (proposal sequence number << 32 | count) into a ring of host memory mapped into the device
// (StepRing, ctx.h), which the host reads with plain loads; an observation below the cap switches back to the exact,
// synchronous path.
// (Until round 3 the read-back was a hipMemcpyAsync into a pinned ring allocated per call plus an event per slot: in
// about one process in four ONE such enqueue stalled for 65-70 ms inside the runtime -- config 4's "slow first
// repetition", DESIGN.md 6 -- and every call paid a hipHostMalloc, four event creations and their release.  The
// sampler's loop now makes no HIP call besides kernel launches and, on the synchronous path, the stream
// synchronisation.)
#pragma once

namespace mcml {

struct StepAhead {
    static constexpr int SLOTS = 8;             // slots of the ring: proposal `seq` writes slot seq % SLOTS
    static constexpr int AHEAD = 4;             // the host runs at most AHEAD proposals ahead of the last count it has seen
    // Speculating costs a whole masked leapfrog step whenever the true count is below the cap (config 5: 290 us against
    // ~30 us for the wait it saves), so it needs evidence: SPEC_STREAK consecutive proposals at the cap, and the first
    // count below it ends it.  (With "the last count seen was at the cap" as the only condition a model whose longest
    // chain hovers round the cap flipped between the two paths by the timing of the read-back: config 5 measured
    // 337-386 ms per iteration from one process to the next on one box.)
    static constexpr int SPEC_STREAK = 8;
    static constexpr double GIVE_UP_MS = 2000.0;    // a count the look-ahead needs and that does not arrive: synchronise
    enum : int { SYNCHRONISE = 0, NOT_ARRIVED = -1, OUT_OF_ORDER = -2 };

    const unsigned long long* ring;             // SLOTS tokens, written by the device
    int cap;                                    // max_steps
    bool allowed;                               // false: always synchronise (GLMMR_MCML_HMC_SPEC=0)
    unsigned last_seq;                          // sequence number of the last proposal launched
    unsigned seen_seq;                          // newest proposal whose count has arrived
    int seen_maxs = -1;                         // latest step count actually observed
    int streak = 0;                             // consecutive proposals observed at the cap

    // seq: the ring's sequence counter as the previous call left it -- this call's proposals continue from seq + 1
    StepAhead(const unsigned long long* ring_, unsigned seq, int cap_, bool allowed_)
        : ring(ring_), cap(cap_), allowed(allowed_), last_seq(seq), seen_seq(seq) {}

    void observe(unsigned sq, int v) { seen_seq = sq; seen_maxs = v; streak = (v == cap) ? streak + 1 : 0; }
    // the counts that have arrived, in proposal order (at most AHEAD + 1 are outstanding); -> how many
    int harvest()
    {
        for (int got = 0;; ++got) {
            const unsigned want = seen_seq + 1;
            if ((int)(last_seq - want) < 0) return got;              // nothing launched beyond what has been seen
            const unsigned long long tok = __atomic_load_n(ring + (want % SLOTS), __ATOMIC_ACQUIRE);
            if ((unsigned)(tok >> 32) != want) return got;           // not there yet
            observe(want, (int)(unsigned)tok);
        }
    }
    // Proposal `seq` and its k_max_steps are on the stream: -> the cap, to launch without waiting, or SYNCHRONISE.
    // now_ms(): a monotonic clock in milliseconds
    template <class Clock>
    int launched(unsigned seq, Clock&& now_ms)
    {
        last_seq = seq;
        harvest();
        if (!allowed || streak < SPEC_STREAK) return SYNCHRONISE;
        // bounded look-ahead: a count below the cap must be noticed within AHEAD proposals (in the dense path a masked
        // step is a full product).  Plain loads of host memory; a count that does not arrive falls back to the wait
        const double t0 = now_ms();
        while ((int)(seq - seen_seq) > AHEAD) {
            harvest();
            if ((int)(seq - seen_seq) > AHEAD && now_ms() - t0 > GIVE_UP_MS) return SYNCHRONISE;
        }
        return streak < SPEC_STREAK ? SYNCHRONISE : cap;
    }
    // After a synchronisation of the stream, slot `seq`: -> the count of proposal `seq`, NOT_ARRIVED if the slot holds
    // another proposal's token, OUT_OF_ORDER unless every count up to and including this one was observed in order
    int synchronised(unsigned seq)
    {
        const unsigned long long tok = __atomic_load_n(ring + (seq % SLOTS), __ATOMIC_ACQUIRE);
        if ((unsigned)(tok >> 32) != seq) return NOT_ARRIVED;
        harvest();
        const int v = (int)(unsigned)tok;
        return (seen_seq == seq && seen_maxs == v) ? v : OUT_OF_ORDER;
    }
};

}  // namespace mcml
