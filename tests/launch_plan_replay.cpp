// launch_plan_replay.cpp -- the pure layer of csrc/gemx_launch_plan.hpp without a GPU (tests/test_launch_plan_cpu.py builds this with a plain
// host compiler and -fsanitize=address,undefined, and runs it).
//   launch_plan_replay <file>   replays every line of a GEMX_PLAN_RECORD file (tests/golden/launch_plans.txt, recorded on an MI355X by
//                               tools/record_launch_plans.py): inputs -> choose_shape / lds_bytes / pace_for, outputs must be equal
//   launch_plan_replay          scripts the closed-loop calibration's decision step with made-up timings
#include <cstdio>
#include <cstring>

#include "gemx_launch_plan.hpp"

using namespace gemx::plan;

// gemx_handle::PaceCal's numbers (gemx_common.hpp), without the event pairs
struct Cal {
    static constexpr int NC = 5, SAMPLES = 6, RING = 16, MAX_RECENTER = 4;
    long long sig = -1;
    float center = 1.0f;
    int recenters = 0, next = 0, chosen = -1;
    float best[NC] = {1e30f, 1e30f, 1e30f, 1e30f, 1e30f};
    int count[NC] = {0, 0, 0, 0, 0}, issued[NC] = {0, 0, 0, 0, 0};
    int ev_cand[RING];
    bool ev_init = true;
    Cal() { for (int i = 0; i < RING; ++i) ev_cand[i] = -1; }
};

static int g_failed = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); ++g_failed; } \
    } while (0)

static int replay(const char *path) {
    FILE *fh = fopen(path, "r");
    if (fh == nullptr) { printf("cannot open %s\n", path); return 2; }
    static const int dummy = 0;
    char line[2048];
    int rows = 0, bad = 0;
    while (fgets(line, sizeof(line), fh) != nullptr) {
        if (line[0] == '#' || line[0] == '\n') continue;
        Facts f = {};
        Launch l = {};
        int b[16], built[NSHAPE], pos = 0, n = 0;
        const char *p = line;
        if (sscanf(p, "%d %d %d %d %d %d %d %d %d %d %d%n", &f.abytes, &f.nht, &f.nact_c, &f.vt_bytes, &f.prep_q, &f.init_desc_bytes, &b[0], &b[1], &b[2], &b[3], &b[4], &n) != 11) { ++bad; continue; }
        p += n;
        f.dq = b[0]; f.compact_l = b[1]; f.sync = b[2]; f.deep_built = b[3]; f.d3_built = b[4];
        bool ok = true;
        for (int s = 0; s < NSHAPE && ok; ++s) {
            ok = sscanf(p, " %d %d %d%n", &built[s], &l.regs[s], &l.occ[s], &n) == 3;
            p += n;
            f.kernel[s] = built[s] ? &dummy : nullptr;
        }
        long long blocks = 0, res = 0;
        size_t lds_max = 0, lds = 0;
        double scale = 1.0;
        int shape = 0, D = 0, OW = 0;
        unsigned bt = 0, tt = 0, tf = 0;
        if (!ok || sscanf(p, " %lld %d %d %d %d %d %d %zu %d %d %d %d %d %d %d %d %d %lg %lg -> %d %d %d %zu %u %u %u %lld%n", &blocks, &l.K, &l.n_cu, &l.nout, &l.delay, &l.rw_n_ref,
                          &l.forced_shape, &lds_max, &b[0], &b[1], &b[2], &b[3], &b[4], &b[5], &b[6], &b[7], &b[8], &l.pace_gbps, &scale, &shape, &D, &OW, &lds, &bt, &tt, &tf, &res, &pos) != 27) { ++bad; continue; }
        l.blocks = blocks; l.lds_max = lds_max;
        l.dq_processor = b[0]; l.need_full = b[1]; l.fast_step = b[2]; l.rinit = b[3]; l.lin_on = b[4]; l.reward = b[5]; l.half = b[6]; l.synth = b[7]; l.pace_default_on = b[8];
        ++rows;
        const Choice c = choose_shape(f, l);
        const Pace pc = pace_for(f, l, c, open_loop_target(f, l) * scale);
        const size_t got_lds = lds_bytes(f, l, c.D);
        if (c.shape != shape || c.D != D || c.OW != OW || got_lds != lds || pc.block_ticks != bt || pc.tail_ticks != tt || pc.tail_from != tf || pc.res != res) {
            printf("row %d differs: recorded shape %d D %d OW %d lds %zu ticks %u %u from %u res %lld, planned shape %d D %d OW %d lds %zu ticks %u %u from %u res %lld\n", rows, shape, D, OW,
                   lds, bt, tt, tf, res, c.shape, c.D, c.OW, got_lds, pc.block_ticks, pc.tail_ticks, pc.tail_from, (long long)pc.res);
            ++g_failed;
        }
    }
    fclose(fh);
    printf("replayed %d rows, %d unreadable, %d differ\n", rows, bad, g_failed);
    return (rows > 0 && bad == 0 && g_failed == 0) ? 0 : 1;
}

// every candidate finishes SAMPLES launches at the given times (ms); returns the turn after the last harvest
static void run_round(Cal &pc, const float (&ms)[Cal::NC]) {
    for (int k = 0; k < Cal::NC * Cal::SAMPLES; ++k) {
        const CalTurn t = cal_turn(pc);
        CHECK(t.slot >= 0);
        cal_harvest(pc, t.slot, ms[t.cand]);
    }
}

static int calibration() {
    {  // candidates are handed out least-issued first, starting with the built-in target; one free pair each
        Cal pc;
        cal_start(pc, 42);
        for (int k = 0; k < 2 * Cal::NC; ++k) {
            const CalTurn t = cal_turn(pc);
            CHECK(t.slot == k && t.cand == k % Cal::NC);
            CHECK(cal_scale(pc, t) == CAL_SCALE[k % Cal::NC] * 1.0f);
        }
        CHECK(pc.next == 2 * Cal::NC);
        for (int k = 2 * Cal::NC; k < Cal::RING; ++k) CHECK(cal_turn(pc).slot == k);
        const CalTurn none = cal_turn(pc);  // no free pair: the starting point, untimed
        CHECK(none.slot < 0 && cal_scale(pc, none) == 1.0);
        cal_harvest(pc, 3, 0.0f);  // (no valid time: the pair is free again, nothing counted)
        CHECK(pc.count[3] == 0 && pc.ev_cand[3] == -1 && cal_turn(pc).slot == 3);
    }
    {  // a candidate replaces the starting point only if it is MORE than 1 % faster
        Cal pc;
        cal_start(pc, 1);
        const float close[Cal::NC] = {1.0f, 0.995f, 1.2f, 1.2f, 1.2f};
        run_round(pc, close);
        CHECK(cal_turn(pc).slot < 0 && pc.chosen == 0);
        Cal pd;
        cal_start(pd, 1);
        const float faster[Cal::NC] = {1.0f, 0.98f, 1.2f, 1.2f, 1.2f};
        run_round(pd, faster);
        const CalTurn t = cal_turn(pd);
        CHECK(t.slot < 0 && pd.chosen == 1 && pd.recenters == 0);
        CHECK(cal_scale(pd, t) == CAL_SCALE[1] * 1.0f);
        Cal pe;  // the unpaced candidate may win as well
        cal_start(pe, 1);
        const float unpaced[Cal::NC] = {1.0f, 1.0f, 1.0f, 1.0f, 0.5f};
        run_round(pe, unpaced);
        CHECK(cal_turn(pe).slot < 0 && pe.chosen == 4 && cal_scale(pe, CalTurn{-1, 0}) == 0.0);
    }
    for (int edge = 2; edge <= 3; ++edge) {  // a winner at x 1.07 or x 0.86 re-centres the bracket, at most MAX_RECENTER times, and clears every in-flight pair
        Cal pc;
        cal_start(pc, 7);
        float ms[Cal::NC] = {1.0f, 1.0f, 1.0f, 1.0f, 1.0f};
        ms[edge] = 0.5f;
        float center = 1.0f;
        for (int r = 0; r < Cal::MAX_RECENTER; ++r) {
            run_round(pc, ms);
            const CalTurn inflight = cal_turn(pc);  // (all counted, so this turn decides: nothing handed out)
            CHECK(inflight.slot < 0);
            center *= (float)CAL_SCALE[edge];
            CHECK(pc.chosen < 0 && pc.recenters == r + 1 && pc.center == center);
            for (int c = 0; c < Cal::NC; ++c) CHECK(pc.best[c] == 1e30f && pc.count[c] == 0 && pc.issued[c] == 0);
            for (int i = 0; i < Cal::RING; ++i) CHECK(pc.ev_cand[i] == -1);
        }
        run_round(pc, ms);
        CHECK(cal_turn(pc).slot < 0 && pc.chosen == edge && pc.recenters == Cal::MAX_RECENTER && pc.center == center);
        CHECK(cal_scale(pc, CalTurn{-1, 0}) == CAL_SCALE[edge] * center);
    }
    {  // re-centring drops the pairs that are still in flight: a stale sample never reaches the new bracket
        Cal pc;
        cal_start(pc, 7);
        const float ms[Cal::NC] = {1.0f, 1.0f, 0.5f, 1.0f, 1.0f};
        for (int k = 0; k < Cal::NC * Cal::SAMPLES; ++k) { const CalTurn t = cal_turn(pc); cal_harvest(pc, t.slot, ms[t.cand]); if (k == 0) { pc.ev_cand[9] = 2; pc.ev_cand[15] = 0; } }
        CHECK(pc.ev_cand[9] == 2 && pc.ev_cand[15] == 0);
        cal_turn(pc);
        CHECK(pc.recenters == 1 && pc.ev_cand[9] == -1 && pc.ev_cand[15] == -1);
    }
    {  // a changed signature starts over; the same one changes nothing
        Cal pc;
        cal_start(pc, 5);
        const float ms[Cal::NC] = {1.0f, 1.0f, 0.5f, 1.0f, 1.0f};
        run_round(pc, ms);
        cal_turn(pc);
        const CalTurn t = cal_turn(pc);
        CHECK(pc.recenters == 1 && t.slot == 0 && pc.issued[0] == 1);
        cal_start(pc, 5);
        CHECK(pc.recenters == 1 && pc.issued[0] == 1 && pc.ev_cand[0] == 0);
        cal_start(pc, 6);
        CHECK(pc.sig == 6 && pc.recenters == 0 && pc.center == 1.0f && pc.chosen == -1 && pc.next == 0 && pc.issued[0] == 0 && pc.ev_cand[0] == -1);
        for (int c = 0; c < Cal::NC; ++c) CHECK(pc.best[c] == 1e30f && pc.count[c] == 0);
    }
    {  // the signature tells launch kinds apart, and K only by its class
        Launch l = {};
        l.blocks = 512; l.K = 64;
        Choice c{1, 4, 2, false};
        const long long s0 = cal_signature(l, c);
        l.K = 255; CHECK(cal_signature(l, c) == s0);
        l.K = 256; CHECK(cal_signature(l, c) != s0);
        l.K = 64; l.reward = true; CHECK(cal_signature(l, c) != s0);
        l.reward = false; l.synth = true; CHECK(cal_signature(l, c) != s0);
        l.synth = false; l.half = true; CHECK(cal_signature(l, c) != s0);
        l.half = false; l.blocks = 513; CHECK(cal_signature(l, c) != s0);
        l.blocks = 512; c.shape = 2; CHECK(cal_signature(l, c) != s0);
        c.shape = 1; c.long_one = true; CHECK(cal_signature(l, c) != s0);
    }
    printf("calibration script: %d failed\n", g_failed);
    return g_failed == 0 ? 0 : 1;
}

int main(int argc, char **argv) { return argc > 1 ? replay(argv[1]) : calibration(); }
