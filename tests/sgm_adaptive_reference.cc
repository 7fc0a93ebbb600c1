// Serial CPU restatement of the adaptive-penalty SGM aggregation (DESIGN.md
// section 3.6, rules A1-A5), written from the rules, not from any other
// implementation: the image is walked LINE BY LINE (a line = the pixels one path
// direction visits in a row, a column or a diagonal), each line keeps only the
// path costs of its previous pixel, and S collects what every line adds.
//
// Every sum is narrowed to 16 bits where rule A2 says so.  Compiled per test
// session by tests/sgm_adaptive_ref.py.
#include <cstdint>
#include <cstdlib>
#include <vector>

namespace {

typedef uint16_t u16;

// A1: the second penalty of one (pixel, predecessor) pair
u16 adapted_penalty(int here, int before, u16 p1, u16 p2)
{
    int const step = std::abs(here - before) + 1;
    int const floor_value = (int)p1 * 3 / 2;
    int const scaled = (int)p2 / step;
    return (u16)(floor_value > scaled ? floor_value : scaled);
}

// A2, literally: every other plane j is looked at for every plane i
void step_literal(const u16* prev, const u16* cost, int D, u16 p1, u16 p2a, u16* out)
{
    u16 lowest = 0xFFFF;
    for (int i = 0; i < D; ++i)
        if (prev[i] < lowest)
            lowest = prev[i];
    for (int i = 0; i < D; ++i) {
        u16 best = prev[i];
        for (int j = 0; j < D; ++j) {
            if (j == i)
                continue;
            int const gap = j > i ? j - i : i - j;
            u16 const cand = (u16)(prev[j] + (gap == 1 ? p1 : p2a));
            if (cand < best)
                best = cand;
        }
        out[i] = (u16)(cost[i] + best - lowest);
    }
}

// A2, closed form (valid where no sum wraps)
void step_closed(const u16* prev, const u16* cost, int D, u16 p1, u16 p2a, u16* out)
{
    u16 lowest = 0xFFFF;
    for (int i = 0; i < D; ++i)
        if (prev[i] < lowest)
            lowest = prev[i];
    for (int i = 0; i < D; ++i) {
        unsigned best = prev[i];
        if (i > 0 && (unsigned)prev[i - 1] + p1 < best)
            best = (unsigned)prev[i - 1] + p1;
        if (i + 1 < D && (unsigned)prev[i + 1] + p1 < best)
            best = (unsigned)prev[i + 1] + p1;
        if (D > 1 && (unsigned)lowest + p2a < best)
            best = (unsigned)lowest + p2a;
        out[i] = (u16)(cost[i] + best - lowest);
    }
}

struct Volume {
    const u16* cost;
    const uint8_t* image;
    int w, h, D;
    u16 p1, p2;
    int literal;
    u16* S;
    const u16* at(int x, int y) const { return cost + ((size_t)y * w + x) * D; }
    u16* sum(int x, int y) const { return S + ((size_t)y * w + x) * D; }
};

// One line of direction (dx, dy) from (x, y); `seeds` = how often the start
// pixel is seeded (A3 / A4: twice on the corner of a diagonal sweep), `stacked`
// = the seeds pile up in the path costs too (A4: the upward sweep only).
void walk(Volume const& V, int x, int y, int dx, int dy, int seeds, bool stacked)
{
    int const D = V.D;
    std::vector<u16> a(D), b(D);
    const u16* c = V.at(x, y);
    u16* s = V.sum(x, y);
    for (int i = 0; i < D; ++i) {
        a[i] = (u16)(stacked ? c[i] * seeds : c[i]);
        s[i] = (u16)(s[i] + c[i] * seeds);
    }
    for (;;) {
        int const nx = x + dx, ny = y + dy;
        if (nx < 0 || nx >= V.w || ny < 0 || ny >= V.h)
            break;
        u16 const p2a = adapted_penalty(V.image[(size_t)ny * V.w + nx],
            V.image[(size_t)y * V.w + x], V.p1, V.p2);
        if (V.literal)
            step_literal(a.data(), V.at(nx, ny), D, V.p1, p2a, b.data());
        else
            step_closed(a.data(), V.at(nx, ny), D, V.p1, p2a, b.data());
        s = V.sum(nx, ny);
        for (int i = 0; i < D; ++i)
            s[i] = (u16)(s[i] + b[i]);
        a.swap(b);
        x = nx;
        y = ny;
    }
}

} // namespace

extern "C" {

// one step of a path: prev[D], cost[D], intensities of the pixel and of its
// predecessor -> out[D]
void sgm_adaptive_ref_step(const uint16_t* prev, const uint16_t* cost, int D, int i1,
    int i2, uint16_t p1, uint16_t p2, int literal, uint16_t* out)
{
    u16 const p2a = adapted_penalty(i1, i2, p1, p2);
    if (literal)
        step_literal(prev, cost, D, p1, p2a, out);
    else
        step_closed(prev, cost, D, p1, p2a, out);
}

uint16_t sgm_adaptive_ref_penalty(int i1, int i2, uint16_t p1, uint16_t p2)
{
    return adapted_penalty(i1, i2, p1, p2);
}

// cost[h][w][D] (u16 holding u8 values), image[h][w] -> S[h][w][D]
void sgm_adaptive_ref_aggregate(const uint16_t* cost, const uint8_t* image, int w, int h,
    int D, uint16_t p1, uint16_t p2, int literal, uint16_t* S)
{
    Volume V = { cost, image, w, h, D, p1, p2, literal, S };
    for (size_t i = 0; i < (size_t)w * h * D; ++i)
        S[i] = 0;
    // the two horizontal sweeps
    for (int y = 0; y < h; ++y) {
        walk(V, 0, y, 1, 0, 1, false);
        walk(V, w - 1, y, -1, 0, 1, false);
    }
    // the downward (dy = 1) and the upward (dy = -1) sweep: a vertical line per
    // column, and for both diagonals a line from every pixel of the entry row
    // and of the entry column; the pixel on both is seeded by both
    for (int dy = 1; dy >= -1; dy -= 2) {
        int const y0 = dy > 0 ? 0 : h - 1;
        bool const stacked = dy < 0;
        for (int x = 0; x < w; ++x)
            walk(V, x, y0, 0, dy, 1, false);
        for (int dx = 1; dx >= -1; dx -= 2) {
            int const x0 = dx > 0 ? 0 : w - 1;
            for (int x = 0; x < w; ++x)
                walk(V, x, y0, dx, dy, x == x0 ? 2 : 1, stacked);
            for (int y = 0; y < h; ++y)
                if (y != y0)
                    walk(V, x0, y, dx, dy, 1, false);
        }
    }
}

} // extern "C"
