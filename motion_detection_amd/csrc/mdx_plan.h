// mdx_plan.h -- what the host decides about memory before a kernel runs, as pure functions: the pyramid
// slab geometry, the class plan of the class-plane LK (residue classes, point order, group shapes,
// A-sum strips, plane layout), the LK scratch layout and a row band's pyramid rows.  A wrong number
// here makes a kernel read outside its planes or read rows nobody built, so nothing in this file
// needs a device: it includes no HIP header and makes no HIP call, builds with a plain C++17 compiler
// and is checked on the CPU (tests/plan_check.cpp).  mdx_internal.h includes it.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

// the functions the kernels share with the host
#ifdef __HIPCC__
#define MDX_HD __host__ __device__
#else
#define MDX_HD
#endif

namespace mdx {

constexpr int kMaxLevels = 8;
constexpr int kWin = 40;     // LK window side (reference optical_flow_calculator.cpp:41)
constexpr int kPad = 40;     // border rows/cols every pyramid level carries (= win)
constexpr int kXOff = 64;    // left margin of a level row: the core starts 64-B aligned

// One pyramid level inside a per-pair slab.  Images are u8; derivatives are uint32 words
// holding (Ix int16 | Iy int16 << 16), the little-endian image of OpenCV's interleaved
// CV_16SC2 derivative Mat.  Both use the same pitch (elements) and origin.
struct Level {
    int w, h;              // core size
    int pitch;             // elements per row (>= kXOff + w + kPad, multiple of 64)
    int rows;              // kPad + h + kPad
    long long img_off;     // byte offset of the level's padded buffer in the u8 slab
    long long der_off;     // word offset of the level's padded buffer in the deriv slab
    MDX_HD long long core() const { return (long long)kPad * pitch + kXOff; }
};

struct Geometry {
    int nlev;                // attained maxLevel + 1
    Level lv[kMaxLevels];
    long long img_bytes;     // bytes of one pyramid slab (all levels)
    long long der_words;     // words of one derivative slab (all levels)
};

// buildOpticalFlowPyramid level count and the padded slab layout for a w x h frame.
inline Geometry make_geometry(int w, int h, int max_level)
{
    Geometry g{};
    int sw = w, sh = h;
    long long img = 0, der = 0;
    int lvl;
    for (lvl = 0; lvl <= max_level; lvl++) {
        Level& L = g.lv[lvl];
        L.w = sw;
        L.h = sh;
        L.pitch = (kXOff + sw + kPad + 16 + 63) / 64 * 64;   // +16: slack for 16-B row loads
        L.rows = kPad + sh + kPad;
        L.img_off = img;
        L.der_off = der;
        img += (long long)L.pitch * L.rows;
        der += (long long)L.pitch * L.rows;
        g.nlev = lvl + 1;
        sw = (sw + 1) / 2;
        sh = (sh + 1) / 2;
        if (sw <= kWin || sh <= kWin) break;
    }
    g.img_bytes = (img + 255) / 256 * 256;
    g.der_words = (der + 63) / 64 * 64;
    return g;
}

// Residue-class planes of LK v2 (mdx_lk.hip): per level, one plane set per class of
// (P_x mod 2^L, P_y mod 2^L) present in the grid.  Each class holds one row-major UH x PW array of
// 8-B (D, C) pairs: D (uint32, Ix | Iy << 16) and C (int32, 256 - 512*I: the J-chain bias, see
// mdx_lk.hip).
struct ClassLevel {
    int nrx, nry;            // residue classes per axis
    int UH, PW;              // plane rows (h + 79), plane width in elements (multiple of 4)
    long long off;           // byte offset of this level inside a pair's class slab
    long long class_bytes;   // UH * PW * 8
    int nxp;                 // length of the padded class-grouped column order (multiple of G)
    int ord_off;             // offset of this level's order tables in LkArgs::ord
    int G;                   // points per LK group (4 or 8)
    int UW;                  // union columns per group (64, 128, 256 or 512)
    int vlo, vhi;            // plane rows the planned grid rows' windows reach (k_lk_class range)
    // A sums per row strip (k_lk_A_rows): the level's grid rows, in class order, cut into strips of
    // at most kAStripRows rows of one y-class whose windows start every `asp` plane rows; 0: the
    // per-group k_lk_A instead (spacing not uniform, or below 5 rows: too many windows overlap)
    int asp;
    int nstrip;              // strips (table at LkArgs::ord + strip_off: (first row index, rows) pairs)
    int strip_off;
};
constexpr int kAStripRows = 16;

// Floor of the LK window origin of grid index gi (column or row) at a level: the reference's
// prevPt * 2^-level - 19.5 in float.  The host plan (which plane rows and columns exist) and the
// kernels (which are read) must agree on it bit for bit: floorf of the same float operands.
MDX_HD inline int lk_win_origin(int gi, int pixel_step, int level)
{
    return (int)floorf((float)(gi * pixel_step) * (float)(1. / (1 << level)) - 19.5f);
}
// First class-plane row of the window with origin row ipy: planes carry kPad rows above the level,
// and a window is clamped into the UH plane rows.
MDX_HD inline int lk_win_row0(int ipy, int UH) { return std::min(std::max(ipy + kPad, 0), UH - kWin); }

// ---------------------------------------------------------------------------------------------
// J - I to float by mantissa bias (the class planes' C word and k_lk_iter's row body, mdx_lk.hip).
// The row body's two dot products give the int32 x = S + 256 - 512*I, of which the reference wants
// jd = x >> 9 as a float.  S is the sum of w*t over the four taps: bytes t, weights w that sum to 16384
// with w00, w01, w10 >= 0 and w11 >= -1, so -255 <= S <= 16385 * 255; I*32 lies in [0, 8160].  Hence
// |x| < 2^22, and with the bias word B = 0x4B400000 (the float 1.5 * 2^23) added -- in the class plane,
// so at no cost in the loop -- the word B + x is the bit pattern of the float 12582912 + x: same
// exponent, 2^22 + x in the mantissa field.  Clearing its low 9 bits floors that field to a multiple of
// 512, which is the float 12582912 + 512 * (x >> 9) (arithmetic shift), and subtracting 12582912.f
// is exact: 512 * jd, by one v_and_b32 and one v_sub_f32 in place of a shift and an integer convert.
// The factor 512 is a power of two and no value comes near overflow or the subnormals
// (|f * fd * 512| <= 4080 * 8160 * 512, below 2.8e13 over a window's 1600 terms), so every product and
// running sum is 512 times the unscaled one with the same roundings; the final scale takes it back.
// tests/lk_jbias_check.cpp checks the identity over the whole range of x.
constexpr uint32_t kLkJBiasWord = 0x4B400000u;   // B: the bit pattern of kLkJBiasFloat
constexpr float kLkJBiasFloat = 12582912.f;      // 1.5 * 2^23
constexpr uint32_t kLkJMask = 0xFFFFFE00u;       // clears the 9 bits the reference shifts out
constexpr int kLkJScale = 512;                   // what lk_jd512's result carries: 2^9
constexpr int kLkJShift = 9;                     // W_BITS1 - 5
constexpr int kLkSMin = -255, kLkSMax = 16385 * 255;   // the four-tap sum S
constexpr int kLkIMax = 8160;                          // I*32 <= 255 * 32
constexpr int kLkXMin = kLkSMin + 256 - 512 * kLkIMax, kLkXMax = kLkSMax + 256;   // x = S + 256 - 512*I
static_assert(16385 * 255 + 256 < (1 << 22), "largest x stays inside the mantissa field's upper half");
static_assert(512 * 8160 + 255 - 256 < (1 << 22), "smallest x stays inside its lower half");
static_assert((kLkJBiasWord & 0x7FFFFFu) == (1u << 22), "the bias puts x = 0 in the middle of the mantissa field");
static_assert(kLkJBiasWord >> 23 == 127 + 23, "exponent 2^23: one mantissa step is 1");
static_assert((1 << kLkJShift) == kLkJScale && kLkJMask == ~(uint32_t)(kLkJScale - 1), "mask, shift and scale agree");
// the class planes' C word: the J-chain rounding bias 256 - 512*I (mdx_lk.hip) plus the bias word
constexpr int kLkCBias = (int)kLkJBiasWord + 256;
MDX_HD inline int lk_class_c(int ival) { return kLkCBias - 512 * ival; }
// the biased dot-product word B + x -> (float)(x >> 9) * 512
MDX_HD inline float lk_jd512(uint32_t biased)
{
    const uint32_t w = biased & kLkJMask;
    float f;
    __builtin_memcpy(&f, &w, sizeof(f));
    return f - kLkJBiasFloat;
}

// (G, UW) shapes of the LK level kernels (mdx_lk.hip instantiates these; the host plan picks the
// smallest UW >= a level's union span among the shapes of its G)
#define LK_SHAPES LK_CASE(4, 48) LK_CASE(4, 56) LK_CASE(4, 64) LK_CASE(4, 72) LK_CASE(4, 80) LK_CASE(4, 96) \
    LK_CASE(4, 128) LK_CASE(8, 80) LK_CASE(8, 112) LK_CASE(8, 128) LK_CASE(8, 256) LK_CASE(8, 512)
constexpr int kLkUW4[] = {48, 56, 64, 72, 80, 96, 128};
constexpr int kLkUW8[] = {80, 112, 128, 256, 512};

struct ClassPlan {
    ClassLevel lv[kMaxLevels];
    long long bytes_per_pair;
    int nch;                 // 0: some group's union is wider than 512 columns (single-kernel LK)
};

// LK counters (queue heads per level and XCD, dataflow retire counts per level and pair): one per
// 128-B line.  Packed, a line held the counters of several levels (or pairs) that concurrently
// running launches update and poll, and the dataflow ran 1.4-3x slower wherever the batch did not
// fill whole lines (8, 16, 24, 40 pairs) -- the concurrent launches contending on shared lines.
constexpr int kCtrPad = 32;
// Dataflow fallback flags of one call (LkArgs::lflags, ints kCtrPad apart, zeroed with the retire
// counters): level l's give-ups (a group wait or the gate before it gave up: the level's results may
// be wrong), whether level l was recomputed (so every finer level must be too), and the queue heads
// of the recompute launches ([level][XCD]).
constexpr int kLkFlagGiveup = 0;
constexpr int kLkFlagRedone = kMaxLevels;
constexpr int kLkFlagQueue = 2 * kMaxLevels;
constexpr int kLkFlagInts = kLkFlagQueue + 8 * kMaxLevels;

// Core rows [lo, hi) of one pyramid level (row-band mode: what a band's LK reads)
struct RowSpan {
    int lo, hi;
};

// ---------------------------------------------------------------------------------------------
// The class plan.  The tables the kernels read (BuiltPlan::tab, uploaded as it stands): the residue
// -> class maps cmap [level][axis][kTabStride] from 0, the class -> residue lists rlist (same shape)
// from kTabRlist, and from kTabOrd every level's order tables: nxp padded grid columns, the band's
// grid rows, the strip pairs (ClassLevel::ord_off, strip_off count from kTabOrd).
constexpr int kTabStride = 128;   // residues per (level, axis): 2^(kMaxLevels - 1)
static_assert(kMaxLevels <= 8, "residue tables sized for 2^7 residues");
constexpr int kTabRlist = kMaxLevels * 2 * kTabStride;
constexpr int kTabOrd = 2 * kTabRlist;

// the context's knobs the plan depends on
struct PlanTuning {
    int lk_g;        // MDX_LK_G: forced group size (4 or 8), 0: per level
    int lk_astrip;   // MDX_LK_ASTRIP: grid rows per A-sum strip, 0: by max_batch
    int max_batch;   // pairs per call the context was made for
};

// Step 1.  One axis' residue classes at a level: the residues (i * ps) mod 2^level of grid indices
// i in [0, cnt), numbered in order of first appearance.  Fills cmap[residue] = class (-1 stays for
// residues the grid never takes) and rlist[class] = residue; returns the number of classes.
inline int residue_classes(int cnt, int ps, int level, int16_t* cmap, int16_t* rlist)
{
    const int m = (1 << level) - 1;
    int n = 0;
    for (int i = 0; i < cnt && n <= m; i++) {
        const int r = (i * ps) & m;
        if (cmap[r] >= 0) continue;
        cmap[r] = (int16_t)n;
        rlist[n++] = (int16_t)r;
    }
    return n;
}

// Step 2.  The columns' class runs: for each of the nrx x-classes, its grid columns in x order.
using ClassRuns = std::vector<std::vector<int16_t>>;
inline ClassRuns class_runs(int nx, int ps, int level, const int16_t* cmx, int nrx)
{
    const int m = (1 << level) - 1;
    ClassRuns runs(nrx);
    for (int i = 0; i < nx; i++) runs[cmx[(i * ps) & m]].push_back((int16_t)i);
    return runs;
}

// Step 3.  The union width of group size G over the runs: the widest span, in level columns, from
// the first member's window origin to the last member's window end, of any group when every run is
// cut into groups of G consecutive members.
inline int union_width(const ClassRuns& runs, int G, int ps, int level)
{
    int u = 0;
    for (const auto& r : runs)
        for (size_t q = 0; q < r.size(); q += G)
            u = std::max(u, lk_win_origin(r[std::min(r.size(), q + G) - 1], ps, level) - lk_win_origin(r[q], ps, level) + kWin);
    return u;
}

// Step 4.  The level's kernel shape from the union widths u4, u8 of groups of 4 and 8: the union
// width is the smallest kernel shape of the group size that fits (0: none does), and the group size
// is 4 (less lockstep) unless 8 stages a row with fewer DMA pieces; forced_g = 4 / 8 (MDX_LK_G)
// forces the group size where a shape fits.  UW == 0: no class-plane kernel for this level.
struct GroupShape {
    int G, UW;
};
inline GroupShape choose_group(int u4, int u8, int forced_g)
{
    auto fit = [](const int* uws, size_t n, int u) {
        for (size_t i = 0; i < n; i++)
            if (uws[i] >= u) return uws[i];
        return 0;
    };
    const int uw4 = fit(kLkUW4, sizeof(kLkUW4) / sizeof(int), u4);
    const int uw8 = fit(kLkUW8, sizeof(kLkUW8) / sizeof(int), u8);
    // a row's staging cost goes by LDS-DMA pieces (1 KiB, one per 64 lanes x 16 B): the
    // wave's union row is 4 slots x uw4 or 2 slots x uw8 pairs of 8 B
    auto pieces = [](int slots, int uw) { return (slots * uw * 8 + 1023) / 1024; };
    const bool g4 = forced_g == 4 ? uw4 > 0
                  : forced_g == 8 ? false
                  : uw4 > 0 && (uw8 == 0 || pieces(4, uw4) <= pieces(2, uw8));
    return g4 ? GroupShape{4, uw4} : GroupShape{8, uw8};
}

// Step 5.  The padded column order, appended to ord: run after run, each padded with -1 to a
// multiple of G, so a group is G consecutive entries of one x-class and starts with its leftmost
// column.  Returns the entries appended (nxp).
inline int append_column_order(const ClassRuns& runs, int G, std::vector<int16_t>& ord)
{
    const size_t o = ord.size();
    for (const auto& r : runs) {
        ord.insert(ord.end(), r.begin(), r.end());
        for (size_t q = r.size(); q % G; q++) ord.push_back((int16_t)-1);
    }
    return (int)(ord.size() - o);
}

// Step 6.  The band's row order, appended to ord: grid rows [gy0, gy1) grouped by y-class, in grid
// order within a class (no padding: a group is one row).
inline void append_row_order(int gy0, int gy1, int ps, int level, const int16_t* cmy, std::vector<int16_t>& ord)
{
    const int m = (1 << level) - 1;
    const size_t r0 = ord.size();
    for (int i = gy0; i < gy1; i++) ord.push_back((int16_t)i);
    std::stable_sort(ord.begin() + r0, ord.end(),
                     [&](int16_t u, int16_t v) { return cmy[(u * ps) & m] < cmy[(v * ps) & m]; });
}

// Step 7.  The A-sum strips (k_lk_A_rows) of a row order (n rows from append_row_order): each run of
// one y-class cut into strips of at most srows rows, as (first index into the row order, rows)
// pairs; and asp, the plane rows between the windows of consecutive rows of a class -- k_lk_A_rows
// needs the spacing uniform over the level and at least 5 rows, else asp = 0 (the per-group k_lk_A).
struct Strips {
    std::vector<int16_t> tab;
    int asp;
};
inline Strips row_strips(const int16_t* rows, size_t n, int ps, int level, const int16_t* cmy, size_t srows)
{
    const int m = (1 << level) - 1;
    Strips S{{}, 0};
    bool uniform = true;
    for (size_t i = 0; i < n;) {
        size_t e = i + 1;
        const int cls = cmy[(rows[i] * ps) & m];
        while (e < n && cmy[(rows[e] * ps) & m] == cls) {
            const int d = lk_win_origin(rows[e], ps, level) - lk_win_origin(rows[e - 1], ps, level);
            if (S.asp == 0) S.asp = d;
            if (d != S.asp) uniform = false;
            e++;
        }
        for (size_t s = i; s < e; s += srows) {
            S.tab.push_back((int16_t)s);
            S.tab.push_back((int16_t)std::min(srows, e - s));
        }
        i = e;
    }
    if (S.asp == 0) S.asp = kWin;   // one row per class: windows never overlap
    if (!uniform || S.asp < 5) S.asp = 0;
    return S;
}
// The strip rows in force.  Small-batch contexts (C4 row bands: one pair per call) take short
// strips: more waves in flight for the few pairs' A sums, which then finish sooner (one band
// 1.196-1.197 against 1.217-1.226 ms at 16, profiles/r05_ab_astrip.txt); at batch 32 4..16 rows
// measured within noise.
inline int strip_rows(const PlanTuning& t) { return t.lk_astrip > 0 ? t.lk_astrip : t.max_batch <= 4 ? 4 : kAStripRows; }

// Step 8.  The plane layout, once every level has its nrx, nry and UW: per level the plane rows UH
// and width PW, the plane rows [vlo, vhi) the band's windows read -- the first rows (lk_win_row0) of
// its first and last grid rows (the window origin is monotone in gy), kWin rows each -- and the
// classes' bytes at ascending offsets; bytes_per_pair covers them.  Returns whether the kernels can
// address a pair's slab: they use 32-bit buffer offsets (the 2 GB rule).
inline bool plane_layout(const Geometry& g, int ps, int gy0, int gy1, ClassPlan& P)
{
    long long off = 0;
    for (int l = 0; l < g.nlev; l++) {
        ClassLevel& C = P.lv[l];
        C.UH = g.lv[l].h + 79;
        C.PW = (g.lv[l].w + kPad + std::max(C.UW, 64) + 3) & ~3;
        C.vlo = lk_win_row0(lk_win_origin(gy0, ps, l), C.UH);
        C.vhi = lk_win_row0(lk_win_origin(gy1 - 1, ps, l), C.UH) + kWin;
        C.class_bytes = (long long)C.UH * C.PW * 8;
        C.off = off;
        off += (long long)C.nrx * C.nry * C.class_bytes;
    }
    P.bytes_per_pair = (off + 255) / 256 * 256;
    return off <= 0x7fff0000LL;
}

// The class plan of grid rows [gy0, gy1) of a w x h frame with geometry g, and its tables.
// plan.nch == 0 means some group's union is wider than 512 columns (pixel_step >~ 66) or a pair's
// class slab exceeds 2 GB: the caller then runs the single-kernel LK instead.
struct BuiltPlan {
    ClassPlan plan;
    std::vector<int16_t> tab;
};
inline BuiltPlan build_class_plan(const Geometry& g, int w, int h, int pixel_step, int gy0, int gy1, const PlanTuning& t)
{
    const int ps = pixel_step, nx = (w + ps - 1) / ps, ny = (h + ps - 1) / ps;
    BuiltPlan B{};
    B.tab.assign(kTabOrd, (int16_t)-1);
    std::vector<int16_t> ord;
    bool usable = true;
    for (int l = 0; l < g.nlev; l++) {
        ClassLevel& C = B.plan.lv[l];
        int16_t* cmx = B.tab.data() + (l * 2 + 0) * kTabStride;
        int16_t* cmy = B.tab.data() + (l * 2 + 1) * kTabStride;
        C.nrx = residue_classes(nx, ps, l, cmx, cmx + kTabRlist);
        C.nry = residue_classes(ny, ps, l, cmy, cmy + kTabRlist);
        const ClassRuns runs = class_runs(nx, ps, l, cmx, C.nrx);
        const GroupShape shape = choose_group(union_width(runs, 4, ps, l), union_width(runs, 8, ps, l), t.lk_g);
        C.G = shape.G;
        C.UW = shape.UW;
        if (C.UW == 0) usable = false;
        C.ord_off = (int)ord.size();
        C.nxp = append_column_order(runs, C.G, ord);
        const size_t r0 = ord.size();
        append_row_order(gy0, gy1, ps, l, cmy, ord);
        const Strips S = row_strips(ord.data() + r0, ord.size() - r0, ps, l, cmy, (size_t)strip_rows(t));
        C.asp = S.asp;
        C.nstrip = (int)S.tab.size() / 2;
        C.strip_off = (int)ord.size();
        ord.insert(ord.end(), S.tab.begin(), S.tab.end());
    }
    if (!plane_layout(g, ps, gy0, gy1, B.plan)) usable = false;
    B.plan.nch = usable ? 1 : 0;
    B.tab.insert(B.tab.end(), ord.begin(), ord.end());
    return B;
}

// ---------------------------------------------------------------------------------------------
// The class-plane LK's scratch (the context's Abuf), byte offsets: the A sums ([level][pair][point] float4,
// from 0), the queue heads ([sub-batch][level][XCD] counters), the dataflow counters and flags
// ([level][pair] + kLkFlagInts counters) and the points carried between levels (per level a
// [pair][point] float2 array of carry_level bytes, a multiple of 128: with the counter regions whole
// 128-B lines and npts a multiple of 16 the arrays start on 128-B lines, which the dataflow requires),
// then the product certificates ([level][pair][point] bytes, written and read with the A sums).
struct LkScratch {
    size_t qctr, done, carry, carry_level, cert, bytes;
};
constexpr size_t kFloat4Bytes = 16;
inline LkScratch lk_scratch(int nlev, int batch, int npts)
{
    LkScratch s;
    s.qctr = (size_t)nlev * batch * npts * kFloat4Bytes;
    s.done = s.qctr + (size_t)batch * kMaxLevels * 8 * kCtrPad * sizeof(int);
    s.carry = s.done + ((size_t)kMaxLevels * batch + kLkFlagInts) * kCtrPad * sizeof(int);
    s.carry_level = ((size_t)batch * npts * 8 + 127) / 128 * 128;
    s.cert = s.carry + s.carry_level * nlev;
    s.bytes = s.cert + (size_t)nlev * batch * npts;
    return s;
}

// Row-band mode: the previous frame's (pyr1) core rows a band's class planes read at each level --
// padded rows [vlo - 1, vhi + 2) of the planes' source (k_lk_class_fused reads y-1 .. y+2, the
// Scharr planes behind k_lk_class the same), reflect-101 border rows folded onto the core rows they
// mirror -- and the rows the next level's pyrDown reads from it (pyramids.cpp: dst row r reads rows
// 2r-2 .. 2r+2).  Only those rows of pyr1 are built; the next frame's pyramid stays whole, since J
// may be read anywhere in it.  rows: [g.nlev].
inline void band_rows(const Geometry& g, const ClassPlan& P, RowSpan* rows)
{
    for (int l = g.nlev - 1; l >= 0; l--) {
        const int h = g.lv[l].h;
        const int lo = P.lv[l].vlo - 1 - kPad, hi = P.lv[l].vhi + 2 - kPad;   // core coordinates
        int clo = std::max(lo, 0), chi = std::min(hi, h);
        if (lo < 0) chi = std::max(chi, std::min(h, 1 - lo));                 // rows lo..-1 mirror 1..-lo
        if (hi > h) clo = std::min(clo, std::max(0, 2 * h - 1 - hi));         // rows h..hi-1 mirror down to 2h-1-hi
        if (l + 1 < g.nlev) {
            clo = std::min(clo, std::max(0, 2 * rows[l + 1].lo - 2));
            chi = std::max(chi, std::min(h, 2 * rows[l + 1].hi + 2));
        }
        rows[l] = RowSpan{clo, std::max(clo, chi)};
    }
}

// Level-0 rows of frame 1 that a band's pyramid build writes, from band_rows' spans (rows[1] must
// be readable: {0, 0} on a one-level pyramid): k_front writes whole level-1 bands, i.e. level-0 rows
// 2*lo1 .. 2*hi1 of the range widened by the level-1 rows wanted.  Within [0, h].
inline RowSpan band_built_rows(const RowSpan* rows, int h)
{
    const int lo1 = std::min(rows[1].lo, rows[0].lo / 2), hi1 = std::max(rows[1].hi, (rows[0].hi + 1) / 2);
    return RowSpan{std::max(0, 2 * lo1), std::min(h, 2 * hi1)};
}

// ---- the border-following rule of the region outlines (mdx_outline.hip), written once for
// the kernels, the host and the CPU test (tests/outline_check.cpp).  Directions d = 0..7 are E, NE, N, NW,
// W, SW, S, SE (x right, y down; increasing d runs counter-clockwise on the screen); bit d of a pixel's
// 8-bit mask is set iff its neighbour in direction d is a member.
MDX_HD inline int outline_dx(int d) { return (d <= 1 || d == 7) - (d >= 3 && d <= 5); }
MDX_HD inline int outline_dy(int d) { return (d >= 5) - (d >= 1 && d <= 3); }
// The step: from state (p, b) -- b the direction from p back to the pixel it was entered from -- the next
// pixel lies in the first direction of b+1, b+2, .., b+8 (mod 8) that holds a member.  -1: no neighbour.
MDX_HD inline int outline_next_dir(unsigned mask, int b)
{
    for (int i = 1; i <= 8; i++)
        if (mask >> ((b + i) & 7) & 1u) return (b + i) & 7;
    return -1;
}
// Its inverse: the state (p, b) whose step leaves p in direction t has b = the first direction of t-1, t-2,
// .., t-8 (mod 8) that holds a member (bit t of mask is set, so there is one).  The start rule is the same
// scan from 3: outline_prev_dir(mask, 4) looks at 3, 2, 1, 0, 7, 6, 5, 4.
MDX_HD inline int outline_prev_dir(unsigned mask, int t)
{
    for (int i = 1; i <= 8; i++)
        if (mask >> ((t - i) & 7) & 1u) return (t - i) & 7;
    return -1;
}
// Rounds of pointer jumping that rank any outline of a w x h image (w * h <= 2^28): ceil(log2) of the bound
// on a position in an outline.  A state is a (pixel, direction) pair and the rule is a bijection on the
// states, so no state occurs twice in an outline; only pixels with a non-member 4-neighbour carry states,
// at most 7 each: fewer than 7 * w * h positions.
inline int outline_rounds(int w, int h)
{
    const long long bound = 7ll * w * h;
    int r = 0;
    while ((1ll << r) < bound) r++;
    return r;
}

}  // namespace mdx
