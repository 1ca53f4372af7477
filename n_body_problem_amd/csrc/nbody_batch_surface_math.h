// nbody_batch_surface_math.h -- the arithmetic of nbody_batch_surface_map (include/nbody_batch_surface.h) that needs no GPU:
// the three records, the six words of one body in the frame and the view (a, b, q, ua, ub, uq), the cell decision on the two
// sets of edges, the 16-bit cell word and the body record, the stable sort of a system's bodies by cell -- the rank step of one
// row over one column, and the detection of the cells' starts in the sorted order -- the walk of one cell's members through
// that order, the walk of total_weight, and the system summary with its peak.  Plain C++17 without HIP, fp64 with +, - and x
// alone: batch_surface_kernel (nbody_batch_analysis.hip) calls these with the image in LDS, and a stand-alone driver
// (tests/batch_surface_driver.cpp) runs whole systems through the same functions, lane by lane for any workgroup shape, on
// the CPU, where tests/test_batch_surface_cpu.py compares every byte with tests/hermite_surface_ref.py.  Nothing here may be
// contracted: the build passes -ffp-contract=off.  Internal; the public surface is include/nbody_batch_surface.h.
#pragma once

#include "nbody_batch_groups_math.h"

namespace nbody {

constexpr int kSurfaceMaxSide = 64;                               // NBODY_BATCH_SURFACE_MAX_SIDE
constexpr int kSurfaceMaxCells = kSurfaceMaxSide * kSurfaceMaxSide;  // 4096: a cell index takes 12 bits
constexpr int kSurfaceOutside = -1, kSurfaceUnmeasured = -2, kSurfaceNotTaking = -3;  // NBODY_BATCH_SURFACE_OUTSIDE ...

// nbody_batch_surface_cell's layout (nbody_batch_analysis.hip asserts it): 64 bytes.
struct BatchSurfaceCell {
    long long count;
    double weight, v1, v2, pa, pb, z1, z2;
};

// nbody_batch_surface_system's layout (nbody_batch_analysis.hip asserts it): 88 bytes.
struct BatchSurfaceSystem {
    int selected, outside, unmeasured, columns, rows, occupied, peak, peak_count;
    double total_weight, centre[3], velocity[3];
};

// nbody_batch_surface_body's layout (nbody_batch_analysis.hip asserts it): 24 bytes.
struct BatchSurfaceBody {
    int cell, reserved;
    double a, b;
};

// ---- Frame, view and edges -------------------------------------------------------------------------------------------------
constexpr double kSurfaceLargest = __DBL_MAX__;

// A finite number: false for NaN and for either infinity; an ordered <= against a finite value, like radial_finite.
NBODY_HD inline bool surface_finite(double v) { return __builtin_fabs(v) <= kSurfaceLargest; }

constexpr int kSurfaceFrameWords = 15;  // centre[3], velocity[3], A[3], B[3], Q[3] of one system
constexpr int kSurfaceViewAt = 6;       // where A starts

// The identity view: A = x, B = y, Q = z.
NBODY_HD inline double surface_identity(int k) { return k == 0 || k == 4 || k == 8 ? 1.0 : 0.0; }

// ---- One body ----------------------------------------------------------------------------------------------------------------
// What the image holds of a body: the position and mass words and the velocity words.
struct SurfacePoint {
    float x, y, z, m, vx, vy, vz;
};

// The body in the frame, rotated into the view.
struct SurfaceWords {
    double a, b, q, ua, ub, uq;
};

// One row vector of the view against a difference: (X_x d_x + X_y d_y) + X_z d_z.
NBODY_HD inline double surface_along(const double *axis, double dx, double dy, double dz)
{
    return (axis[0] * dx + axis[1] * dy) + axis[2] * dz;
}

// frame: centre[3], velocity[3], A[3], B[3], Q[3].
NBODY_HD inline SurfaceWords surface_words(const SurfacePoint &p, const double *frame)
{
    const double dx = (double)p.x - frame[0], dy = (double)p.y - frame[1], dz = (double)p.z - frame[2];
    const double ux = (double)p.vx - frame[3], uy = (double)p.vy - frame[4], uz = (double)p.vz - frame[5];
    const double *A = frame + kSurfaceViewAt, *B = A + 3, *Q = A + 6;
    SurfaceWords w;
    w.a = surface_along(A, dx, dy, dz);
    w.b = surface_along(B, dx, dy, dz);
    w.q = surface_along(Q, dx, dy, dz);
    w.ua = surface_along(A, ux, uy, uz);
    w.ub = surface_along(B, ux, uy, uz);
    w.uq = surface_along(Q, ux, uy, uz);
    return w;
}

// w: the mass word or 1, widened.
NBODY_HD inline double surface_weight(const SurfacePoint &p, int weight) { return weight == kGroupsWeightNumber ? 1.0 : (double)p.m; }

// Measured: all six words are finite.
NBODY_HD inline bool surface_measured(const SurfaceWords &w)
{
    return surface_finite(w.a) && surface_finite(w.b) && surface_finite(w.q) && surface_finite(w.ua) && surface_finite(w.ub) &&
           surface_finite(w.uq);
}

// The bin of a finite v among bins + 1 strictly ascending edges: the edges at or below v are counted, so that bin t is
// e[t] <= v < e[t + 1]; -1 where v < e[0] or v >= e[bins].
NBODY_HD inline int surface_bin(double v, const double *e, int bins)
{
    int passed = 0;
    for (int t = 0; t <= bins; ++t)
        passed += v >= e[t] ? 1 : 0;
    return passed == 0 || passed == bins + 1 ? -1 : passed - 1;
}

// The cell of a body taking part: j * columns + i, or kSurfaceOutside, or kSurfaceUnmeasured.
NBODY_HD inline int surface_cell(const SurfaceWords &w, const double *ea, int columns, const double *eb, int rows)
{
    if (!surface_measured(w))
        return kSurfaceUnmeasured;
    const int i = surface_bin(w.a, ea, columns), j = surface_bin(w.b, eb, rows);
    return i < 0 || j < 0 ? kSurfaceOutside : j * columns + i;
}

// The 16-bit cell word of the image: the cell index 0 ... 4095, or a sentinel above every cell -- 4096 outside, 4097 unmeasured,
// 4098 not taking part -- so that a sentinel never sorts below a member.
constexpr int kSurfaceWordOutside = kSurfaceMaxCells, kSurfaceWordUnmeasured = kSurfaceMaxCells + 1,
              kSurfaceWordNotTaking = kSurfaceMaxCells + 2;
NBODY_HD inline int surface_word(int cell) { return cell >= 0 ? cell : kSurfaceMaxCells - 1 - cell; }
NBODY_HD inline int surface_cell_of_word(int word) { return word < kSurfaceMaxCells ? word : kSurfaceMaxCells - 1 - word; }
NBODY_HD inline bool surface_word_inside(int word) { return word < kSurfaceMaxCells; }
// Whether a cell word is that of a measured body taking part (a member or outside): total_weight's bodies.
NBODY_HD inline bool surface_counts_in_total(int word) { return word <= kSurfaceWordOutside; }

// The body record: the rotated coordinates of a measured body taking part.
NBODY_HD inline BatchSurfaceBody surface_body(int cell, const SurfaceWords &w)
{
    const bool measured = cell >= kSurfaceOutside;
    return BatchSurfaceBody{cell, 0, measured ? w.a : 0.0, measured ? w.b : 0.0};
}
NBODY_HD inline BatchSurfaceBody surface_body_absent() { return BatchSurfaceBody{kSurfaceNotTaking, 0, 0.0, 0.0}; }

// ---- The stable sort by cell -------------------------------------------------------------------------------------------------
// Row i's place in order[] is #{j : word_j < word_i} + #{j < i : word_j == word_i}: the number of bodies whose key
// (word, index) is below its own.  A body index is below 4096 = 2^12, so the key is one 32-bit word and the rank step one
// comparison and one add.
NBODY_HD inline unsigned surface_key(int word, int index) { return ((unsigned)word << 12) | (unsigned)index; }

// The rank step of one row (its key) over one column (body j's cell word): 1 iff body j sorts before the row.
NBODY_HD inline int surface_rank_step(unsigned row_key, int word_j, int j) { return surface_key(word_j, j) < row_key ? 1 : 0; }

// The starts of the cells fall out of the sorted order: place k starts a cell iff it is the first place or the cell before
// it differs.  `here` and `before` are the cell words of order[k] and order[k - 1].
NBODY_HD inline bool surface_is_start(int k, int here, int before) { return k == 0 || here != before; }
constexpr int kSurfaceNoStart = 0xFFFF;  // the start word of an empty cell: no place is 65535

// ---- The walks ---------------------------------------------------------------------------------------------------------------
// One member joins the seven sums: one add per term, the addend w * (...) with the parenthesis first.
NBODY_HD inline void surface_add(BatchSurfaceCell &c, double w, const SurfaceWords &b)
{
    c.weight += w;
    c.v1 += w * b.uq;
    c.v2 += w * (b.uq * b.uq);
    c.pa += w * b.ua;
    c.pb += w * b.ub;
    c.z1 += w * b.q;
    c.z2 += w * (b.q * b.q);
}

// The walker of cell c goes through order[] from the cell's start while the cell word is c: its members in ascending body
// index, because the sort is stable.  Image: word(j), the cell word of body j; point(j), its SurfacePoint; order(k), the body
// at place k; start(c), the place where cell c starts or kSurfaceNoStart.  m: the number of places.  Without `sums` only the
// count is formed (a call that asks for no cell records needs it for occupied and peak).
template <class Image>
NBODY_HD inline BatchSurfaceCell surface_walk(const Image &img, int m, int c, const double *frame, int weight, bool sums)
{
    BatchSurfaceCell cell{};
    const int first = img.start(c);
    if (first == kSurfaceNoStart)
        return cell;
    for (int k = first; k < m; ++k) {
        const int j = img.order(k);
        if (img.word(j) != c)
            break;
        cell.count += 1;
        if (sums) {
            const SurfacePoint p = img.point(j);
            surface_add(cell, surface_weight(p, weight), surface_words(p, frame));
        }
    }
    return cell;
}

// total_weight: w of every measured body taking part, outside ones included, j = 0 ... n - 1.
template <class Image>
NBODY_HD inline double surface_walk_total(const Image &img, int n, int weight)
{
    double sum = 0.0;
    for (int j = 0; j < n; ++j)
        if (surface_counts_in_total(img.word(j)))
            sum += surface_weight(img.point(j), weight);
    return sum;
}

// ---- The system summary ------------------------------------------------------------------------------------------------------
// The peak of a system as one word that an integer maximum reduces: the larger count wins and, among equal counts, the lower
// cell.  0: no occupied cell.  count <= 4096 takes 13 bits, the cell 12.
NBODY_HD inline unsigned surface_peak_key(long long count, int cell)
{
    return count > 0 ? ((unsigned)count << 12) | (unsigned)(kSurfaceMaxCells - 1 - cell) : 0u;
}

NBODY_HD inline BatchSurfaceSystem surface_system(int selected, int outside, int unmeasured, int columns, int rows, int occupied,
                                                  unsigned peak_key, double total, const double *frame)
{
    const int peak = peak_key ? kSurfaceMaxCells - 1 - (int)(peak_key & (kSurfaceMaxCells - 1)) : -1;
    return BatchSurfaceSystem{selected, outside, unmeasured, columns, rows, occupied, peak, (int)(peak_key >> 12), total,
                              {frame[0], frame[1], frame[2]}, {frame[3], frame[4], frame[5]}};
}

}  // namespace nbody
