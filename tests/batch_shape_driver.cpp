// Runs whole systems through the arithmetic of csrc/nbody_batch_shape_math.h (include/nbody_batch_shape.h) on the CPU for
// tests/test_batch_shape_cpu.py: the functions batch_shape_kernel calls, in the kernel's phases and for the kernel's
// assignment of rows, apertures and blocks to lanes -- a workgroup of T lanes (a multiple of 64) with RPL rows per lane at
// r = q * T + tid, wave w of the T / 64 taking the apertures w, w + T / 64, ..., lane k of that wave walking block k, and
// every lane adding the block partials for itself -- through an image laid out as the kernel's, shift included.
// Commands on stdin:
//   system N SLOTS T RPL APERTURES WEIGHT REDUCED MAX_ITERATIONS MIN_MEMBERS WANT -> then one line with tol, one line of
//                    APERTURES radii, one of APERTURES inner radii, one line of the frame (centre[3], velocity[3]) and N lines
//                    "x y z m vx vy vz take" (numbers read as double by strtod, so that hexadecimal floats, nan and inf are
//                    read; the body's words are narrowed to float).  WANT 0: no aperture records are asked for.  Prints three
//                    lines of hexadecimal bytes: the system record; the APERTURES aperture records (empty without WANT); the
//                    SLOTS body records.
//   layout        -> the sizes of the three records and the offsets of their fields
#include "nbody_batch_shape_math.h"

#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

using namespace nbody;

static double read_double(std::istream &in)
{
    std::string w;
    in >> w;
    return std::strtod(w.c_str(), nullptr);
}

static void print_bytes(const void *data, size_t bytes)
{
    const unsigned char *p = static_cast<const unsigned char *>(data);
    for (size_t k = 0; k < bytes; ++k)
        std::printf("%02x", p[k]);
    std::printf("\n");
}

// The image as the kernel keeps it: two 16-byte words per body at shape_image_slot.
struct Word {
    float v[4];
};
struct Image {
    const std::vector<Word> *words;
    ShapePoint point(int i) const
    {
        const Word &p = words->at((size_t)shape_image_slot(i)), &v = words->at((size_t)shape_image_slot(i) + 1);
        return ShapePoint{p.v[0], p.v[1], p.v[2], p.v[3], v.v[0], v.v[1], v.v[2]};
    }
};

static int run_system(std::istringstream &in)
{
    int n = 0, slots = 0, T = 0, rpl = 0, apertures = 0, weight = 0, reduced = 0, max_iterations = 0, min_members = 0, want = 0;
    in >> n >> slots >> T >> rpl >> apertures >> weight >> reduced >> max_iterations >> min_members >> want;
    if (n < 0 || n > slots || T < 64 || T % 64 || rpl < 1 || rpl * T < slots || apertures < 1 || apertures > kShapeMaxApertures ||
        (weight != kGroupsWeightMass && weight != kGroupsWeightNumber) || max_iterations < 1 || max_iterations > kShapeMaxIterations ||
        min_members < kShapeLeastMembers || shape_blocks(n) > 64) {
        std::fprintf(stderr, "system: bad arguments\n");
        return 2;
    }
    std::string line;
    std::getline(std::cin, line);
    std::istringstream tol_words(line);
    const double tol = read_double(tol_words);
    std::vector<double> ap((size_t)apertures * kShapeApertureWords);
    for (int part = 0; part < 2; ++part) {
        std::getline(std::cin, line);
        std::istringstream words(line);
        for (int a = 0; a < apertures; ++a)
            ap[(size_t)a * kShapeApertureWords + (size_t)part] = read_double(words);
    }
    for (int a = 0; a < apertures; ++a) {
        double *w = ap.data() + (size_t)a * kShapeApertureWords;
        if (!shape_finite(w[0]) || !(w[0] > 0.0) || !(w[1] >= 0.0) || !(w[1] < w[0]) || !shape_finite(tol) || tol < 0.0) {
            std::fprintf(stderr, "system: bad aperture\n");
            return 2;
        }
        w[2] = shape_square(w[0]);
        w[3] = shape_square(w[1]);
    }
    std::getline(std::cin, line);
    std::istringstream frame_words(line);
    double frame[kShapeFrameWords];
    for (double &f : frame)
        f = read_double(frame_words);
    std::vector<ShapePoint> points((size_t)(n > 0 ? n : 1));
    std::vector<char> take((size_t)(n > 0 ? n : 1), 1);
    for (int i = 0; i < n; ++i) {
        std::getline(std::cin, line);
        std::istringstream words(line);
        ShapePoint &p = points[(size_t)i];
        p.x = (float)read_double(words);
        p.y = (float)read_double(words);
        p.z = (float)read_double(words);
        p.m = (float)read_double(words);
        p.vx = (float)read_double(words);
        p.vy = (float)read_double(words);
        p.vz = (float)read_double(words);
        int t = 1;
        words >> t;
        take[(size_t)i] = t != 0;
    }
    // Phase 1: the lanes in any order -- here descending, to make the point -- every row its words in the image.
    std::vector<Word> words((size_t)shape_image_slots(slots));
    std::memset(words.data(), 0xAB, sizeof(Word) * words.size());
    std::vector<unsigned char> inside((size_t)shape_inside_bytes(slots), 0);
    int tally[3] = {0, 0, 0};
    for (int tid = T - 1; tid >= 0; --tid)
        for (int q = 0; q < rpl; ++q) {
            const int r = q * T + tid;
            if (r >= n)
                continue;
            const ShapePoint &given = points[(size_t)r];
            const bool takes = take[(size_t)r] != 0, measured = shape_measured(given);
            tally[0] += takes ? 1 : 0;
            tally[1] += takes && !measured ? 1 : 0;
            const ShapePoint held = shape_image_point(given, takes && measured);
            words[(size_t)shape_image_slot(r)] = Word{{held.x, held.y, held.z, held.m}};
            words[(size_t)shape_image_slot(r) + 1] = Word{{held.vx, held.vy, held.vz, 0.f}};
        }
    const Image image{&words};
    const int waves = T / 64, blocks = shape_blocks(n);
    // total_weight: wave 0, lane k block k, then every lane the level-2 sum (lane 0's is kept).
    double total_weight = 0.0;
    {
        ShapePartial<1> part[64] = {};
        for (int lane = 63; lane >= 0; --lane)
            for (int i = lane * kShapeBlock; i < shape_block_end(lane, n); ++i)
                shape_total_step(part[lane], image.point(i), weight);
        total_weight = shape_level2<1>([&](int k) { return part[k]; }, blocks).v[0];
    }
    std::vector<BatchShapeAperture> records((size_t)apertures);
    std::memset(records.data(), 0xAB, sizeof(BatchShapeAperture) * records.size());
    for (int wave = waves - 1; wave >= 0; --wave)
        for (int a = wave; a < apertures; a += waves) {
            const double *w = ap.data() + (size_t)a * kShapeApertureWords;
            // Every lane of the wave carries the iteration for itself; they must agree, and lane 0's record is written.
            ShapeProgress g = shape_start();
            for (int pass = 0; pass < kShapeMaxIterations && !g.done; ++pass) {
                ShapePartial<kShapePassWords> part[64] = {};
                for (int lane = 63; lane >= 0; --lane)
                    for (int i = lane * kShapeBlock; i < shape_block_end(lane, n); ++i)
                        shape_pass_step(part[lane], image.point(i), frame, g.state, w[3], w[2], weight, reduced != 0);
                ShapeProgress next = g;
                for (int lane = 63; lane >= 0; --lane) {
                    ShapeProgress mine = g;
                    shape_update(mine, shape_level2<kShapePassWords>([&](int k) { return part[k]; }, blocks), tol, max_iterations,
                                 min_members);
                    if (lane != 63 && std::memcmp(&mine.state, &next.state, sizeof mine.state) != 0) {
                        std::fprintf(stderr, "system: the lanes disagree\n");
                        return 3;
                    }
                    next = mine;
                }
                g = next;
            }
            ShapePartial<kShapeFinalWords> part[64] = {};
            for (int lane = 63; lane >= 0; --lane)
                for (int i = lane * kShapeBlock; i < shape_block_end(lane, n); ++i)
                    if (shape_final_step(part[lane], image.point(i), frame, g.state, w[3], w[2], weight))
                        inside.at((size_t)shape_inside_at(i)) |= (unsigned char)(1u << a);
            records[(size_t)a] = shape_record(g, w[0], w[1], shape_level2<kShapeFinalWords>([&](int k) { return part[k]; }, blocks));
            tally[2] += g.status == kShapeConverged ? 1 : 0;
        }
    std::vector<BatchShapeBody> bodies((size_t)slots);
    for (int r = 0; r < slots; ++r)
        bodies[(size_t)r] = shape_body(r < n ? inside.at((size_t)shape_inside_at(r)) : 0u);
    const BatchShapeSystem s = shape_system(tally[0], tally[1], apertures, reduced != 0 ? 1 : 0, tally[2], total_weight, frame);
    print_bytes(&s, sizeof s);
    print_bytes(records.data(), want ? sizeof(BatchShapeAperture) * records.size() : 0);
    print_bytes(bodies.data(), sizeof(BatchShapeBody) * bodies.size());
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
            std::printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu", sizeof(BatchShapeAperture),
                        offsetof(BatchShapeAperture, status), offsetof(BatchShapeAperture, iterations), offsetof(BatchShapeAperture, count),
                        offsetof(BatchShapeAperture, radius), offsetof(BatchShapeAperture, inner), offsetof(BatchShapeAperture, q),
                        offsetof(BatchShapeAperture, s), offsetof(BatchShapeAperture, change), offsetof(BatchShapeAperture, eigenvalues),
                        offsetof(BatchShapeAperture, axes), offsetof(BatchShapeAperture, weight), offsetof(BatchShapeAperture, D),
                        offsetof(BatchShapeAperture, M), offsetof(BatchShapeAperture, L));
            std::printf(" %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu", sizeof(BatchShapeSystem), offsetof(BatchShapeSystem, selected),
                        offsetof(BatchShapeSystem, unmeasured), offsetof(BatchShapeSystem, apertures), offsetof(BatchShapeSystem, reduced),
                        offsetof(BatchShapeSystem, converged), offsetof(BatchShapeSystem, reserved), offsetof(BatchShapeSystem, total_weight),
                        offsetof(BatchShapeSystem, centre), offsetof(BatchShapeSystem, velocity));
            std::printf(" %zu %zu %zu\n", sizeof(BatchShapeBody), offsetof(BatchShapeBody, inside), offsetof(BatchShapeBody, reserved));
        } else {
            std::fprintf(stderr, "unknown command %s\n", word.c_str());
            return 2;
        }
    }
    return 0;
}
