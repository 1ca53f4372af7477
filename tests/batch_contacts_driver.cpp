// Runs whole systems through the arithmetic of csrc/nbody_batch_contacts_math.h (include/nbody_batch_contacts.h) on the CPU for
// tests/test_batch_contacts_cpu.py: the functions batch_contacts_kernel calls, in the kernel's three phases and for the
// kernel's assignment of rows to lanes -- a workgroup of T lanes (a multiple of 64) with RPL rows per lane at r = q * T + tid --
// so that the placement runs over the units (q, wave) as it does on the device.
// Commands on stdin:
//   system N SLOTS T RPL MODE CAPACITY RADIUS ALWAYS -> then N lines "x y z R take" (numbers read as double, narrowed to
//                    float).  MODE 0: radius mode with RADIUS; MODE 1: radii mode with the R of every line.  ALWAYS 1: every wave
//                    repeats the walk for the fill; 0: a wave with nothing to write skips it.  Prints three lines:
//                    bodies touching max_degree reserved pairs stored closest_i closest_j bits(closest_r2) reserved2;
//                    degree upper first nearest of every slot;  i j bits(r2) of every list entry (empty at CAPACITY 0).
//   layout        -> the sizes of the three records and the offsets of their fields
#include "nbody_batch_contacts_math.h"

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
    float x, y, z, w;  // w: the radius, a NaN where the body takes no part (radii mode); the take-part flag (radius mode)
    bool take;
};

static int run_system(std::istringstream &in)
{
    int n = 0, slots = 0, T = 0, rpl = 0, mode = 0, always = 0;
    long long capacity = 0;
    in >> n >> slots >> T >> rpl >> mode >> capacity;
    const float radius = read_float(in);
    in >> always;
    if (n < 0 || n > slots || T < kContactsWave || T % kContactsWave || rpl < 1 || rpl * T < slots || capacity < 0) {
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
        p.x = read_float(words);
        p.y = read_float(words);
        p.z = read_float(words);
        const float R = read_float(words);
        int take = 1;
        words >> take;
        p.take = take != 0;
        p.w = radii ? (p.take ? R : contacts_no_radius()) : (p.take ? 1.f : 0.f);
        taking += p.take ? 1 : 0;
    }
    const int waves = T / kContactsWave, rows = rpl * T;
    const auto t2_of = [&](int r, int j) { return radii ? contacts_radii_t2(body[(size_t)r].w, body[(size_t)j].w) : b2; };
    const auto r2_of = [&](int r, int j) {
        return groups_r2(body[(size_t)r].x, body[(size_t)r].y, body[(size_t)r].z, body[(size_t)j].x, body[(size_t)j].y, body[(size_t)j].z);
    };
    // Count: the lanes in any order -- here descending, to make the point -- every row over every column.
    std::vector<ContactRow> row((size_t)rows);
    int touching = 0, max_degree = 0;
    SpanKey closest = kSpanNoKey;
    for (int tid = T - 1; tid >= 0; --tid)
        for (int q = 0; q < rpl; ++q) {
            const int r = q * T + tid;
            if (r < n)
                for (int j = 0; j < n; ++j) {
                    if (!radii && !body[(size_t)j].take)
                        continue;
                    contacts_step(row[(size_t)r], contacts_examined(body[(size_t)r].take, true, r, j), r, j, r2_of(r, j), t2_of(r, j));
                }
            touching += row[(size_t)r].degree >= 1 ? 1 : 0;
            max_degree = row[(size_t)r].degree > max_degree ? row[(size_t)r].degree : max_degree;
            const SpanKey key = contacts_row_key(row[(size_t)r], r);
            closest = key < closest ? key : closest;
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
    const BatchContactSystem s = contacts_system(taking, touching, max_degree, pairs, capacity, closest);
    // Fill: wave by wave, from the column above the wave's first row on; then the pads.  Every entry starts out as a value
    // that neither a contact nor a pad holds, so that a place nobody wrote shows.
    std::vector<BatchContact> list((size_t)capacity, BatchContact{-7, -7, -7.f});
    if (capacity > 0) {
        for (int wave = waves - 1; wave >= 0; --wave) {
            bool fills = false;
            for (int lane = 0; lane < kContactsWave; ++lane)
                for (int q = 0; q < rpl; ++q) {
                    const int r = q * T + wave * kContactsWave + lane;
                    fills = fills || contacts_row_fills(first[(size_t)r], row[(size_t)r].upper, capacity);
                }
            if (!always && !fills)
                continue;
            for (int lane = 0; lane < kContactsWave; ++lane)
                for (int q = 0; q < rpl; ++q) {
                    const int r = q * T + wave * kContactsWave + lane;
                    int t = 0;
                    if (r < n)
                        for (int j = wave * kContactsWave + 1; j < n; ++j) {
                            if (!radii && !body[(size_t)j].take)
                                continue;
                            contacts_fill(list.data(), capacity, first[(size_t)r], t, contacts_examined(body[(size_t)r].take, true, r, j), r,
                                          j, r2_of(r, j), t2_of(r, j));
                        }
                }
        }
        for (long long k = contacts_stored(pairs, capacity); k < capacity; ++k)
            list[(size_t)k] = contacts_pad();
    }
    std::printf("%d %d %d %d %lld %lld %d %d %u %d\n", s.bodies, s.touching, s.max_degree, s.reserved, s.pairs, s.stored, s.closest_i,
                s.closest_j, float_bits(s.closest_r2), s.reserved2);
    for (int r = 0; r < slots; ++r) {
        const BatchContactBody rec = contacts_body(row[(size_t)r], first[(size_t)r]);
        std::printf("%s%d %d %d %d", r ? " " : "", rec.degree, rec.upper, rec.first, rec.nearest);
    }
    std::printf("\n");
    for (long long k = 0; k < capacity; ++k)
        std::printf("%s%d %d %u", k ? " " : "", list[(size_t)k].i, list[(size_t)k].j, float_bits(list[(size_t)k].r2));
    std::printf("\n");
    return 0;
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
        } else if (word == "layout") {
            std::printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(BatchContactSystem),
                        offsetof(BatchContactSystem, bodies), offsetof(BatchContactSystem, touching),
                        offsetof(BatchContactSystem, max_degree), offsetof(BatchContactSystem, reserved),
                        offsetof(BatchContactSystem, pairs), offsetof(BatchContactSystem, stored),
                        offsetof(BatchContactSystem, closest_i), offsetof(BatchContactSystem, closest_j),
                        offsetof(BatchContactSystem, closest_r2), offsetof(BatchContactSystem, reserved2), sizeof(BatchContactBody),
                        offsetof(BatchContactBody, degree), offsetof(BatchContactBody, upper), offsetof(BatchContactBody, first),
                        offsetof(BatchContactBody, nearest), sizeof(BatchContact), offsetof(BatchContact, i), offsetof(BatchContact, j),
                        offsetof(BatchContact, r2));
        } else {
            std::fprintf(stderr, "unknown command %s\n", word.c_str());
            return 2;
        }
    }
    return 0;
}
