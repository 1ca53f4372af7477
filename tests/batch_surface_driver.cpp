// Runs whole systems through the arithmetic of csrc/nbody_batch_surface_math.h (include/nbody_batch_surface.h) on the CPU for
// tests/test_batch_surface_cpu.py: the functions batch_surface_kernel calls, in the kernel's three phases and for the kernel's
// assignment of rows and cells to lanes -- a workgroup of T lanes (a multiple of 64) with RPL rows per lane at r = q * T + tid,
// and the walker of cell c = tid, tid + T, ...  The arrays are the kernel's LDS arrays with the kernel's sizes, so that an
// index the kernel would put out of bounds is one here too, where the address sanitizer sees it.
// Commands on stdin:
//   system N SLOTS T RPL COLUMNS ROWS WEIGHT WANT -> then one line of COLUMNS + 1 edges, one of ROWS + 1 edges, one line of the
//                    frame (centre[3], velocity[3], A[3], B[3], Q[3]) and N lines "x y z m vx vy vz take" (numbers read as
//                    double by strtod, so that hexadecimal floats, nan and inf are read; the body's words are narrowed to
//                    float).  WANT 0: no cell records are asked for.  Prints three lines of hexadecimal bytes: the system
//                    record; the COLUMNS x ROWS cell records (empty without WANT); the SLOTS body records.  Every cell
//                    record starts out as a pattern that no walker writes, so that a record nobody wrote shows.
//   layout        -> the sizes of the three records and the offsets of their fields
#include "nbody_batch_surface_math.h"

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

// The image as the kernel keeps it: the bodies' words and the three arrays of 16-bit words.
struct Image {
    const std::vector<SurfacePoint> *points;
    const std::vector<unsigned short> *words, *places, *starts;
    int word(int j) const { return words->at((size_t)j); }
    int order(int k) const { return places->at((size_t)k); }
    int start(int c) const { return starts->at((size_t)c); }
    SurfacePoint point(int j) const { return points->at((size_t)j); }
};

static int run_system(std::istringstream &in)
{
    int n = 0, slots = 0, T = 0, rpl = 0, columns = 0, rows = 0, weight = 0, want = 0;
    in >> n >> slots >> T >> rpl >> columns >> rows >> weight >> want;
    if (n < 0 || n > slots || slots < 1 || slots > 4096 || T < 64 || T % 64 || rpl < 1 || rpl * T < slots || columns < 1 ||
        columns > kSurfaceMaxSide || rows < 1 || rows > kSurfaceMaxSide || (weight != kGroupsWeightMass && weight != kGroupsWeightNumber)) {
        std::fprintf(stderr, "system: bad arguments\n");
        return 2;
    }
    std::string line;
    std::vector<double> ea((size_t)columns + 1), eb((size_t)rows + 1);
    for (std::vector<double> *e : {&ea, &eb}) {
        std::getline(std::cin, line);
        std::istringstream edge_words(line);
        for (double &v : *e)
            v = read_double(edge_words);
    }
    std::getline(std::cin, line);
    std::istringstream frame_words(line);
    double frame[kSurfaceFrameWords];
    for (double &f : frame)
        f = read_double(frame_words);
    std::vector<SurfacePoint> points((size_t)slots);
    std::vector<char> take((size_t)slots, 1);
    for (int i = 0; i < n; ++i) {
        std::getline(std::cin, line);
        std::istringstream words(line);
        SurfacePoint &p = points[(size_t)i];
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
    const int cells = columns * rows, padded = (slots + 7) / 8 * 8;
    // Phase 1: the lanes in any order -- here descending, to make the point -- every row its cell word and its body record.
    std::vector<unsigned short> cell_of((size_t)padded, 0xDEAD), order((size_t)padded, 0xDEAD), starts((size_t)cells, kSurfaceNoStart);
    std::vector<BatchSurfaceBody> bodies((size_t)slots);
    std::vector<unsigned> key((size_t)rpl * (size_t)T);
    int tally[3] = {0, 0, 0};
    for (int tid = T - 1; tid >= 0; --tid)
        for (int q = 0; q < rpl; ++q) {
            const int r = q * T + tid;
            BatchSurfaceBody record = surface_body_absent();
            int word = kSurfaceWordNotTaking;
            if (r < n && take[(size_t)r]) {
                const SurfaceWords b = surface_words(points[(size_t)r], frame);
                const int cell = surface_cell(b, ea.data(), columns, eb.data(), rows);
                word = surface_word(cell);
                tally[0] += 1;
                tally[1] += cell == kSurfaceOutside ? 1 : 0;
                tally[2] += cell == kSurfaceUnmeasured ? 1 : 0;
                record = surface_body(cell, b);
            }
            if (r < padded)
                cell_of.at((size_t)r) = (unsigned short)word;
            key[(size_t)q * (size_t)T + (size_t)tid] = surface_key(word, r);
            if (r < slots)
                bodies[(size_t)r] = record;
        }
    const int m = tally[0] - tally[1] - tally[2];
    // Phase 2: the rank walk of every row over the columns 0 ... the eight that holds n - 1, then the starts.
    for (int tid = T - 1; tid >= 0; --tid)
        for (int q = 0; q < rpl; ++q) {
            const int r = q * T + tid;
            const unsigned mine = key[(size_t)q * (size_t)T + (size_t)tid];
            int rank = 0;
            for (int j = 0; j < (n + 7) / 8 * 8; ++j)
                rank += surface_rank_step(mine, cell_of.at((size_t)j), j);
            if (r < n && surface_word_inside((int)(mine >> 12)))
                order.at((size_t)rank) = (unsigned short)r;  // at(): a rank beyond the array is an error here
        }
    for (int k = m - 1; k >= 0; --k) {
        const int here = cell_of.at(order.at((size_t)k)), before = k > 0 ? cell_of.at(order.at((size_t)k - 1)) : here;
        if (surface_is_start(k, here, before))
            starts.at((size_t)here) = (unsigned short)k;
    }
    // Phase 3: the walkers of every lane, the lanes descending again; the integer reductions; lane 0 adds total_weight.
    std::vector<BatchSurfaceCell> records((size_t)cells);
    std::memset(records.data(), 0xAB, sizeof(BatchSurfaceCell) * records.size());
    const Image image{&points, &cell_of, &order, &starts};
    int occupied = 0;
    unsigned peak = 0;
    double total = 0.0;
    for (int tid = T - 1; tid >= 0; --tid) {
        for (int c = tid; c < cells; c += T) {
            const BatchSurfaceCell cell = surface_walk(image, m, c, frame, weight, want != 0);
            if (want)
                records[(size_t)c] = cell;
            occupied += cell.count > 0 ? 1 : 0;
            const unsigned mine = surface_peak_key(cell.count, c);
            peak = mine > peak ? mine : peak;
        }
        if (tid == 0)
            total = surface_walk_total(image, n, weight);
    }
    const BatchSurfaceSystem s = surface_system(tally[0], tally[1], tally[2], columns, rows, occupied, peak, total, frame);
    print_bytes(&s, sizeof s);
    print_bytes(records.data(), want ? sizeof(BatchSurfaceCell) * records.size() : 0);
    print_bytes(bodies.data(), sizeof(BatchSurfaceBody) * bodies.size());
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
            std::printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu", sizeof(BatchSurfaceCell), offsetof(BatchSurfaceCell, count),
                        offsetof(BatchSurfaceCell, weight), offsetof(BatchSurfaceCell, v1), offsetof(BatchSurfaceCell, v2),
                        offsetof(BatchSurfaceCell, pa), offsetof(BatchSurfaceCell, pb), offsetof(BatchSurfaceCell, z1),
                        offsetof(BatchSurfaceCell, z2));
            std::printf(" %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu", sizeof(BatchSurfaceSystem), offsetof(BatchSurfaceSystem, selected),
                        offsetof(BatchSurfaceSystem, outside), offsetof(BatchSurfaceSystem, unmeasured), offsetof(BatchSurfaceSystem, columns),
                        offsetof(BatchSurfaceSystem, rows), offsetof(BatchSurfaceSystem, occupied), offsetof(BatchSurfaceSystem, peak),
                        offsetof(BatchSurfaceSystem, peak_count), offsetof(BatchSurfaceSystem, total_weight),
                        offsetof(BatchSurfaceSystem, centre), offsetof(BatchSurfaceSystem, velocity));
            std::printf(" %zu %zu %zu %zu %zu\n", sizeof(BatchSurfaceBody), offsetof(BatchSurfaceBody, cell),
                        offsetof(BatchSurfaceBody, reserved), offsetof(BatchSurfaceBody, a), offsetof(BatchSurfaceBody, b));
        } else {
            std::fprintf(stderr, "unknown command %s\n", word.c_str());
            return 2;
        }
    }
    return 0;
}
