// Runs whole systems through the arithmetic of csrc/nbody_batch_approaches_math.h (include/nbody_batch_approaches.h) on the CPU
// for tests/test_batch_approaches_cpu.py: the functions batch_approaches_kernel calls, in the kernel's three steps (count,
// place, fill) and for the kernel's assignment of rows to lanes -- a workgroup of T lanes (a multiple of 64) with RPL rows per
// lane at r = q * T + tid -- so that the placement runs over the units (q, wave) as it does on the device.
// Commands on stdin:
//   system N SLOTS T RPL MODE CAPACITY RADIUS H ALWAYS END -> then N lines "x y z vx vy vz R take" (numbers read as double,
//                    narrowed to float).  MODE 0: radius mode with RADIUS; MODE 1: radii mode with the R of every line.  ALWAYS
//                    1: every wave repeats the walk for the fill; 0: a wave with nothing to write skips it.  END 1: the
//                    separation at the horizon is computed for every pair; 0: only for a pair that is decided there, and a NaN
//                    is passed for every other.  Prints three lines:
//                    bodies approaching max_degree reserved pairs stored now passing ending reserved2;
//                    degree upper first now of every slot;  i j bits(r2) bits(rv) bits(v2) phase of every list entry.
//   pair DX DY DZ WX WY WZ T2 H -> the phase of one pair at d and w, with the first body at rest at the origin, and the bits of
//                    r2, rv and v2, both ways round (the second as the first would be from the other body)
//   layout        -> the sizes of the three records and the offsets of their fields
#include "nbody_batch_approaches_math.h"

#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

using namespace nbody;

static unsigned float_bits(float f)
{
    unsigned w;
    std::memcpy(&w, &f, sizeof w);
    return w;
}

static float read_float(std::istream &in)
{
    std::string w;
    in >> w;
    return (float)std::strtod(w.c_str(), nullptr);
}

struct Body {
    ApproachPoint p;
    float radius;  // a NaN where the body takes no part (radii mode); 0 in radius mode
    bool take;
};

static int run_system(std::istringstream &in)
{
    int n = 0, slots = 0, T = 0, rpl = 0, mode = 0, always = 0, end = 0;
    long long capacity = 0;
    in >> n >> slots >> T >> rpl >> mode >> capacity;
    const float radius = read_float(in), h = read_float(in);
    in >> always >> end;
    if (n < 0 || n > slots || T < kContactsWave || T % kContactsWave || rpl < 1 || rpl * T < slots || capacity < 0 ||
        !approaches_horizon_valid(h)) {
        std::fprintf(stderr, "system: bad arguments\n");
        return 2;
    }
    const bool radii = mode != 0;
    const float b2 = contacts_radius_t2(radius);
    std::vector<Body> body((size_t)(n > 0 ? n : 1));
    std::string line;
    int taking = 0;
    for (int i = 0; i < n; ++i) {
        std::getline(std::cin, line);
        std::istringstream words(line);
        Body &p = body[(size_t)i];
        p.p.x = read_float(words);
        p.p.y = read_float(words);
        p.p.z = read_float(words);
        p.p.vx = read_float(words);
        p.p.vy = read_float(words);
        p.p.vz = read_float(words);
        const float R = read_float(words);
        int take = 1;
        words >> take;
        p.take = take != 0;
        p.radius = radii ? (p.take ? R : contacts_no_radius()) : 0.f;
        taking += p.take ? 1 : 0;
    }
    const int waves = T / kContactsWave, rows = rpl * T;
    const auto t2_of = [&](int r, int j) { return radii ? contacts_radii_t2(body[(size_t)r].radius, body[(size_t)j].radius) : b2; };
    // One pair as the kernel sees it: the words, then the phase with m2 where it is computed.
    const auto phase_of = [&](int r, int j, ApproachWords &words) {
        const ApproachPoint &a = body[(size_t)r].p, &c = body[(size_t)j].p;
        words = approaches_words(a, c);
        const float t2 = t2_of(r, j);
        const bool reach = end || approaches_ends(words, t2, h);
        return approaches_phase(words, t2, h, reach ? approaches_m2(a, c, h) : __builtin_nanf(""));
    };
    // Count: the lanes in any order -- here descending, to make the point -- every row over every column.
    std::vector<ApproachRow> row((size_t)rows);
    int approaching = 0, max_degree = 0;
    int phases[kApproachPhases] = {0, 0, 0};
    for (int tid = T - 1; tid >= 0; --tid)
        for (int q = 0; q < rpl; ++q) {
            const int r = q * T + tid;
            if (r < n)
                for (int j = 0; j < n; ++j) {
                    if (!body[(size_t)j].take)
                        continue;
                    ApproachWords words;
                    const int phase = phase_of(r, j, words);
                    approaches_step(row[(size_t)r], phases, contacts_examined(body[(size_t)r].take, true, r, j), r, j, phase);
                }
            approaching += row[(size_t)r].degree >= 1 ? 1 : 0;
            max_degree = row[(size_t)r].degree > max_degree ? row[(size_t)r].degree : max_degree;
        }
    // Place: inside a unit (q, wave) the lanes in ascending order from a running sum that starts at 0; then the units below.
    std::vector<int> totals((size_t)(rpl * waves)), first((size_t)rows);
    for (int q = 0; q < rpl; ++q)
        for (int wave = 0; wave < waves; ++wave) {
            int running = 0;
            for (int lane = 0; lane < kContactsWave; ++lane) {
                const int r = q * T + wave * kContactsWave + lane;
                first[(size_t)r] = contacts_place(running, row[(size_t)r].upper);
            }
            totals[(size_t)contacts_unit(q, waves, wave)] = running;
        }
    for (int q = 0; q < rpl; ++q)
        for (int tid = 0; tid < T; ++tid)
            first[(size_t)(q * T + tid)] += contacts_units_below(totals.data(), contacts_unit(q, waves, tid / kContactsWave));
    const long long pairs = contacts_units_below(totals.data(), rpl * waves);
    const BatchApproachSystem s = approaches_system(taking, approaching, max_degree, pairs, capacity, phases[kApproachNow],
                                                    phases[kApproachPassage], phases[kApproachEnd]);
    // Fill: wave by wave, from the column above the wave's first row on; then the pads.  Every entry starts out as a value
    // that neither an approach nor a pad holds, so that a place nobody wrote shows.
    std::vector<BatchApproach> list((size_t)capacity, BatchApproach{-7, -7, -7.f, -7.f, -7.f, -7});
    if (capacity > 0) {
        for (int wave = waves - 1; wave >= 0; --wave) {
            bool fills = false;
            for (int lane = 0; lane < kContactsWave; ++lane)
                for (int q = 0; q < rpl; ++q) {
                    const int r = q * T + wave * kContactsWave + lane;
                    fills = fills || approaches_row_fills(first[(size_t)r], row[(size_t)r].upper, capacity);
                }
            if (!always && !fills)
                continue;
            for (int lane = 0; lane < kContactsWave; ++lane)
                for (int q = 0; q < rpl; ++q) {
                    const int r = q * T + wave * kContactsWave + lane;
                    int t = 0;
                    if (r < n)
                        for (int j = wave * kContactsWave + 1; j < n; ++j) {
                            if (!body[(size_t)j].take)
                                continue;
                            ApproachWords words;
                            const int phase = phase_of(r, j, words);
                            approaches_fill(list.data(), capacity, first[(size_t)r], t, contacts_examined(body[(size_t)r].take, true, r, j),
                                            r, j, words, phase);
                        }
                }
        }
        for (long long k = contacts_stored(pairs, capacity); k < capacity; ++k)
            list[(size_t)k] = approaches_pad();
    }
    std::printf("%d %d %d %d %lld %lld %d %d %d %d\n", s.bodies, s.approaching, s.max_degree, s.reserved, s.pairs, s.stored, s.now,
                s.passing, s.ending, s.reserved2);
    for (int r = 0; r < slots; ++r) {
        const BatchApproachBody rec = approaches_body(row[(size_t)r], first[(size_t)r]);
        std::printf("%s%d %d %d %d", r ? " " : "", rec.degree, rec.upper, rec.first, rec.now);
    }
    std::printf("\n");
    for (long long k = 0; k < capacity; ++k) {
        const BatchApproach &e = list[(size_t)k];
        std::printf("%s%d %d %u %u %u %d", k ? " " : "", e.i, e.j, float_bits(e.r2), float_bits(e.rv), float_bits(e.v2), e.phase);
    }
    std::printf("\n");
    return 0;
}

static void run_pair(std::istringstream &in)
{
    float w[6];
    for (float &v : w)
        v = read_float(in);
    const float t2 = read_float(in), h = read_float(in);
    const ApproachPoint a{0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, c{w[0], w[1], w[2], w[3], w[4], w[5]};
    const ApproachPoint *ends[2][2] = {{&a, &c}, {&c, &a}};
    for (int k = 0; k < 2; ++k) {
        const ApproachWords p = approaches_words(*ends[k][0], *ends[k][1]);
        const int phase = approaches_phase(p, t2, h, approaches_m2(*ends[k][0], *ends[k][1], h));
        std::printf("%s%d %u %u %u", k ? " " : "", phase, float_bits(p.r2), float_bits(p.rv), float_bits(p.v2));
    }
    std::printf("\n");
}

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string word;
        if (!(in >> word))
            continue;
        if (word == "system") {
            if (const int status = run_system(in))
                return status;
        } else if (word == "pair") {
            run_pair(in);
        } else if (word == "layout") {
            std::printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n",
                        sizeof(BatchApproachSystem), offsetof(BatchApproachSystem, bodies), offsetof(BatchApproachSystem, approaching),
                        offsetof(BatchApproachSystem, max_degree), offsetof(BatchApproachSystem, reserved),
                        offsetof(BatchApproachSystem, pairs), offsetof(BatchApproachSystem, stored), offsetof(BatchApproachSystem, now),
                        offsetof(BatchApproachSystem, passing), offsetof(BatchApproachSystem, ending),
                        offsetof(BatchApproachSystem, reserved2), sizeof(BatchApproachBody), offsetof(BatchApproachBody, degree),
                        offsetof(BatchApproachBody, upper), offsetof(BatchApproachBody, first), offsetof(BatchApproachBody, now),
                        sizeof(BatchApproach), offsetof(BatchApproach, i), offsetof(BatchApproach, j), offsetof(BatchApproach, r2),
                        offsetof(BatchApproach, rv), offsetof(BatchApproach, v2), offsetof(BatchApproach, phase));
        } else {
            std::fprintf(stderr, "unknown command %s\n", word.c_str());
            return 2;
        }
    }
    return 0;
}
