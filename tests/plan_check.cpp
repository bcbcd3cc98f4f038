// plan_check.cpp -- the host plan of the class-plane LK (motion_detection_amd/csrc/mdx_plan.h) run on a
// CPU: builds the plans of tests/test_class_plan.py's configurations, checks by brute force over every
// grid point that no kernel would read outside its planes or rows nobody built, and prints every plan
// as one JSON document (stdout) for the comparison with tests/golden/class_plan_parent.json.
// Violations go to stderr; the exit status is 1 when there was one.
//   g++ -std=c++17 -I motion_detection_amd/csrc -I include tests/plan_check.cpp
#include "mdx_plan.h"

#include <cstdio>
#include <string>
#include <vector>

using namespace mdx;

static int g_fail = 0;
static std::string g_where;
#define CHECK(cond, ...)                                                      \
    do {                                                                      \
        if (!(cond) && ++g_fail <= 40) {                                      \
            fprintf(stderr, "FAIL [%s] %s: ", g_where.c_str(), #cond);        \
            fprintf(stderr, __VA_ARGS__);                                     \
            fputc('\n', stderr);                                              \
        }                                                                     \
    } while (0)

struct Config {
    int w, h, ps, max_level;
    int gy0, gy1;   // grid rows of the band; gy1 < 0: every row
    PlanTuning t;
};

static int clampi(int v, int lo, int hi) { return std::min(std::max(v, lo), hi); }
// reflect-101 of core row y onto [0, h)
static int reflect101(int y, int h)
{
    if (h == 1) return 0;
    while (y < 0 || y >= h) y = y < 0 ? -y : 2 * h - 2 - y;
    return y;
}

// Columns, rows, strips and layout of one usable plan (the issue's invariants).
static void check_plan(const Config& c, const Geometry& g, const BuiltPlan& B, int gy0, int gy1)
{
    const ClassPlan& P = B.plan;
    const int ps = c.ps, nx = (c.w + ps - 1) / ps, nyb = gy1 - gy0;
    const int srows = c.t.lk_astrip > 0 ? c.t.lk_astrip : c.t.max_batch <= 4 ? 4 : kAStripRows;
    long long end = 0;
    for (int l = 0; l < g.nlev; l++) {
        const ClassLevel& C = P.lv[l];
        const int m = (1 << l) - 1, lw = g.lv[l].w;
        g_where += " L" + std::to_string(l);
        // the tables lie inside what is uploaded
        const long long tabn = (long long)B.tab.size() - kTabOrd;
        const bool inside = C.ord_off >= 0 && C.nxp >= 0 && (long long)C.ord_off + C.nxp + nyb <= C.strip_off &&
                            C.nstrip >= 0 && (long long)C.strip_off + 2 * C.nstrip <= tabn;
        CHECK(inside, "ord_off %d nxp %d nyb %d strip_off %d nstrip %d of %lld", C.ord_off, C.nxp, nyb, C.strip_off, C.nstrip, tabn);
        if (!inside) return;
        const int16_t* cmx = B.tab.data() + (l * 2 + 0) * kTabStride;
        const int16_t* cmy = B.tab.data() + (l * 2 + 1) * kTabStride;
        const int16_t* ord = B.tab.data() + kTabOrd + C.ord_off;
        const int16_t* rows = ord + C.nxp;
        const int16_t* strips = B.tab.data() + kTabOrd + C.strip_off;
        auto xcls = [&](int gx) { return (int)cmx[(gx * ps) & m]; };
        auto ycls = [&](int gy) { return (int)cmy[(gy * ps) & m]; };
        // residue tables: class and residue are each other's inverse
        for (int axis = 0; axis < 2; axis++) {
            const int16_t* cm = axis ? cmy : cmx;
            const int ncls = axis ? C.nry : C.nrx, cnt = axis ? (c.h + ps - 1) / ps : nx;
            for (int i = 0; i < cnt; i++) {
                const int r = (i * ps) & m, k = cm[r];
                CHECK(k >= 0 && k < ncls && cm[kTabRlist + k] == r, "axis %d index %d residue %d class %d", axis, i, r, k);
            }
        }
        // the shape is one the kernels are instantiated for
        bool shape = false;
#define LK_CASE(G_, UW_) shape = shape || (C.G == G_ && C.UW == UW_);
        LK_SHAPES
#undef LK_CASE
        CHECK(shape, "(G, UW) = (%d, %d)", C.G, C.UW);
        // columns
        CHECK(C.G > 0 && C.nxp % C.G == 0, "nxp %d G %d", C.nxp, C.G);
        std::vector<int> seen(nx, 0);
        for (int i = 0; i < C.nxp; i++) {
            CHECK(ord[i] >= -1 && ord[i] < nx, "ord[%d] = %d", i, ord[i]);
            if (ord[i] >= 0 && ord[i] < nx) seen[ord[i]]++;
        }
        for (int gx = 0; gx < nx; gx++) CHECK(seen[gx] == 1, "column %d listed %d times", gx, seen[gx]);
        for (int k = 0; k + C.G <= C.nxp; k += C.G) {
            const int first = ord[k];
            CHECK(first >= 0, "group %d starts with padding", k / C.G);
            if (first < 0) continue;
            const int ub = clampi(lk_win_origin(first, ps, l) + kPad, 0, C.PW - C.UW);
            CHECK(0 <= ub && ub + C.UW <= C.PW, "group %d: union [%d, +%d) of PW %d", k / C.G, ub, C.UW, C.PW);
            for (int j = 0; j < C.G; j++) {
                const int gx = ord[k + j];
                if (gx < 0) continue;
                CHECK(j == 0 || gx > first, "group %d: member %d left of the first %d", k / C.G, gx, first);
                CHECK(xcls(gx) == xcls(first), "group %d: members %d and %d in two x-classes", k / C.G, first, gx);
                const int o = lk_win_origin(gx, ps, l);
                if (o >= -kWin && o < lw)
                    CHECK(0 <= o + kPad - ub && o + kPad - ub <= C.UW - kWin, "group %d column %d: window at %d of union [%d, +%d)",
                          k / C.G, gx, o + kPad, ub, C.UW);
            }
        }
        // rows: each once, contiguous by y-class, windows inside [vlo, vhi)
        std::vector<int> rseen(std::max(nyb, 0), 0), cls_done(C.nry, 0);
        for (int i = 0; i < nyb; i++) {
            const int gy = rows[i];
            CHECK(gy >= gy0 && gy < gy1, "row order [%d] = %d", i, gy);
            if (gy < gy0 || gy >= gy1) continue;
            rseen[gy - gy0]++;
            if (i > 0 && ycls(rows[i - 1]) != ycls(gy)) cls_done[ycls(rows[i - 1])] = 1;
            CHECK(!cls_done[ycls(gy)], "y-class %d not contiguous at row order [%d]", ycls(gy), i);
            const int v0 = lk_win_row0(lk_win_origin(gy, ps, l), C.UH);
            CHECK(0 <= C.vlo && C.vlo <= v0 && v0 + kWin <= C.vhi && C.vhi <= C.UH, "row %d: window rows [%d, +40) of [%d, %d) of %d",
                  gy, v0, C.vlo, C.vhi, C.UH);
            if (C.asp != 0 && i > 0 && ycls(rows[i - 1]) == ycls(gy))
                CHECK(lk_win_origin(gy, ps, l) - lk_win_origin(rows[i - 1], ps, l) == C.asp, "rows %d, %d not asp %d apart",
                      rows[i - 1], gy, C.asp);
        }
        for (int i = 0; i < nyb; i++) CHECK(rseen[i] == 1, "row %d listed %d times", gy0 + i, rseen[i]);
        // strips tile the row order, each inside one y-class
        int pos = 0;
        for (int s = 0; s < C.nstrip; s++) {
            const int first = strips[2 * s], len = strips[2 * s + 1];
            CHECK(first == pos && len >= 1 && len <= srows && first + len <= nyb, "strip %d = (%d, %d) at %d, strip rows %d", s, first,
                  len, pos, srows);
            if (first != pos || len < 1 || first + len > nyb) break;
            for (int i = 1; i < len; i++) CHECK(ycls(rows[first + i]) == ycls(rows[first]), "strip %d spans two y-classes", s);
            pos += len;
        }
        CHECK(pos == nyb, "strips cover %d of %d rows", pos, nyb);
        if (C.asp != 0) CHECK((C.asp >= 10 ? 4 : 8) * C.asp >= kWin, "asp %d: window slots wrap (launch_A_rows)", C.asp);
        // layout
        CHECK(C.UH == g.lv[l].h + 79 && C.PW % 4 == 0 && C.class_bytes == (long long)C.UH * C.PW * 8, "UH %d PW %d class_bytes %lld",
              C.UH, C.PW, C.class_bytes);
        CHECK(C.off >= end, "off %lld overlaps the level above, which ends at %lld", C.off, end);
        end = C.off + (long long)C.nrx * C.nry * C.class_bytes;
        g_where.resize(g_where.rfind(" L"));
    }
    CHECK(P.bytes_per_pair % 256 == 0 && P.bytes_per_pair >= end && end <= 0x7fff0000LL, "bytes_per_pair %lld, levels end at %lld",
          P.bytes_per_pair, end);
}

// band_rows' spans hold every pyramid row the band's planes and the coarser levels' pyrDown read;
// band_built_rows contains level 0's.
static void check_band_rows(const Config& c, const Geometry& g, const ClassPlan& P, const RowSpan* rows, RowSpan built)
{
    for (int l = 0; l < g.nlev; l++) {
        const int h = g.lv[l].h;
        CHECK(0 <= rows[l].lo && rows[l].lo <= rows[l].hi && rows[l].hi <= h, "level %d span [%d, %d) of %d", l, rows[l].lo, rows[l].hi, h);
        const int p0 = std::max(P.lv[l].vlo - 1, 0), p1 = std::min(P.lv[l].vhi + 2, g.lv[l].rows);
        for (int p = p0; p < p1; p++) {
            const int y = reflect101(p - kPad, h);
            CHECK(rows[l].lo <= y && y < rows[l].hi, "level %d padded row %d -> core %d outside [%d, %d)", l, p, y, rows[l].lo, rows[l].hi);
        }
        if (l + 1 < g.nlev)
            for (int r = rows[l + 1].lo; r < rows[l + 1].hi; r++)
                for (int k = -2; k <= 2; k++) {
                    const int y = reflect101(2 * r + k, h);
                    CHECK(rows[l].lo <= y && y < rows[l].hi, "level %d row %d reads level %d row %d outside [%d, %d)", l + 1, r, l, y,
                          rows[l].lo, rows[l].hi);
                }
    }
    CHECK(0 <= built.lo && built.lo <= rows[0].lo && rows[0].hi <= built.hi && built.hi <= c.h, "built [%d, %d), level 0 [%d, %d) of %d",
          built.lo, built.hi, rows[0].lo, rows[0].hi, c.h);
}

static void run_config(const Config& c, bool first)
{
    char name[160];
    snprintf(name, sizeof(name), "%dx%d ps %d ml %d rows [%d, %d) g %d astrip %d batch %d", c.w, c.h, c.ps, c.max_level, c.gy0, c.gy1,
             c.t.lk_g, c.t.lk_astrip, c.t.max_batch);
    g_where = name;
    const Geometry g = make_geometry(c.w, c.h, c.max_level);
    const int ny = (c.h + c.ps - 1) / c.ps, gy0 = c.gy0, gy1 = c.gy1 < 0 ? ny : c.gy1;
    const BuiltPlan B = build_class_plan(g, c.w, c.h, c.ps, gy0, gy1, c.t);
    const ClassPlan& P = B.plan;
    printf("%s\n{\"cfg\":[%d,%d,%d,%d,%d,%d,%d,%d,%d],\"nlev\":%d,\"nch\":%d,\"bytes_per_pair\":%lld,\"lv\":[", first ? "" : ",", c.w, c.h,
           c.ps, c.max_level, c.gy0, c.gy1, c.t.lk_g, c.t.lk_astrip, c.t.max_batch, g.nlev, P.nch, P.bytes_per_pair);
    for (int l = 0; l < g.nlev; l++) {
        const ClassLevel& C = P.lv[l];
        printf("%s{\"nrx\":%d,\"nry\":%d,\"UH\":%d,\"PW\":%d,\"off\":%lld,\"class_bytes\":%lld,\"nxp\":%d,\"ord_off\":%d,\"G\":%d,\"UW\":%d,"
               "\"vlo\":%d,\"vhi\":%d,\"asp\":%d,\"nstrip\":%d,\"strip_off\":%d}",
               l ? "," : "", C.nrx, C.nry, C.UH, C.PW, C.off, C.class_bytes, C.nxp, C.ord_off, C.G, C.UW, C.vlo, C.vhi, C.asp, C.nstrip,
               C.strip_off);
    }
    printf("]");
    if (P.nch != 0) {
        check_plan(c, g, B, gy0, gy1);
        RowSpan rows[kMaxLevels] = {};
        band_rows(g, P, rows);
        const RowSpan built = band_built_rows(rows, c.h);
        check_band_rows(c, g, P, rows, built);
        printf(",\"rows\":[");
        for (int l = 0; l < g.nlev; l++) printf("%s[%d,%d]", l ? "," : "", rows[l].lo, rows[l].hi);
        printf("],\"built\":[%d,%d]", built.lo, built.hi);
    }
    // the uploaded tables, int16 by int16, low byte first
    printf(",\"tab\":\"");
    for (int16_t v : B.tab) printf("%02x%02x", (unsigned)v & 0xff, ((unsigned)v >> 8) & 0xff);
    printf("\"}");
}

// lk_scratch: regions in order without overlap, carried points on 128-B lines, `done` as large as
// what lk_enqueue_iters clears.
static void run_scratch(int nlev, int batch, int npts, bool first)
{
    char name[96];
    snprintf(name, sizeof(name), "lk_scratch(%d, %d, %d)", nlev, batch, npts);
    g_where = name;
    const LkScratch s = lk_scratch(nlev, batch, npts);
    const size_t pts = (size_t)nlev * batch * npts;
    CHECK(s.qctr >= pts * 16, "A sums end at %zu", s.qctr);
    CHECK(s.done >= s.qctr + (size_t)batch * kMaxLevels * 8 * kCtrPad * sizeof(int), "queue heads [%zu, %zu)", s.qctr, s.done);
    CHECK(s.carry - s.done == ((size_t)kMaxLevels * batch + kLkFlagInts) * kCtrPad * sizeof(int) && s.carry > s.done, "done [%zu, %zu)",
          s.done, s.carry);
    CHECK(s.carry_level >= (size_t)batch * npts * 8 && s.cert >= s.carry + s.carry_level * nlev, "carry %zu x %d from %zu, cert at %zu",
          s.carry_level, nlev, s.carry, s.cert);
    CHECK(s.bytes >= s.cert + pts, "cert [%zu, %zu)", s.cert, s.bytes);
    if (npts % 16 == 0)
        for (int l = 0; l < nlev; l++) CHECK((s.carry + l * s.carry_level) % 128 == 0, "level %d's carried points at %zu", l, s.carry + l * s.carry_level);
    printf("%s\n{\"args\":[%d,%d,%d],\"qctr\":%zu,\"done\":%zu,\"carry\":%zu,\"carry_level\":%zu,\"cert\":%zu,\"bytes\":%zu}", first ? "" : ",",
           nlev, batch, npts, s.qctr, s.done, s.carry, s.carry_level, s.cert, s.bytes);
}

int main()
{
    // the smallest shapes at which each rule of the plan is reached (tests/test_class_plan.py says which)
    struct Shape {
        int w, h, ps, max_level;
    };
    const Shape shapes[] = {{41, 41, 1, 5},      {72, 72, 3, 5},     {100, 100, 1, 5},    {164, 244, 10, 5},  {4864, 164, 10, 5},
                            {320, 240, 10, 5},   {320, 240, 10, 0},  {320, 240, 10, 7},   {330, 250, 10, 5},  {640, 480, 7, 5},
                            {640, 480, 16, 5},   {1280, 720, 33, 5}, {1920, 1080, 10, 5}, {1920, 1080, 64, 5}, {1920, 1080, 70, 5},
                            {3840, 2160, 10, 5}};
    std::vector<Config> cfgs;
    for (const Shape& s : shapes)
        for (int lk_g : {0, 4, 8})
            for (int max_batch : {1, 32}) cfgs.push_back({s.w, s.h, s.ps, s.max_level, 0, -1, {lk_g, 0, max_batch}});
    for (int astrip : {1, 64}) {
        cfgs.push_back({1920, 1080, 10, 5, 0, -1, {0, astrip, 32}});
        cfgs.push_back({330, 250, 10, 5, 0, -1, {0, astrip, 1}});
    }
    // row bands (contexts made for one pair): 1080p's 108 grid rows cut in 2, 3, 4, 8 and 108 pieces
    for (int pieces : {2, 3, 4, 8, 108})
        for (int max_batch : {1, 32})
            for (int k = 0; k < pieces; k++) {
                if (pieces == 108 && max_batch == 32) continue;
                cfgs.push_back({1920, 1080, 10, 5, 108 * k / pieces, 108 * (k + 1) / pieces, {0, 0, max_batch}});
            }
    cfgs.push_back({320, 240, 10, 5, 3, 4, {0, 0, 1}});

    printf("{\"plans\":[");
    for (size_t i = 0; i < cfgs.size(); i++) run_config(cfgs[i], i == 0);
    printf("\n],\"scratch\":[");
    bool first = true;
    for (int nlev : {1, 3, 5, 6, 8})
        for (int batch : {1, 3, 8, 32})
            for (int npts : {1, 7, 16, 768, 20736, 82944}) {
                run_scratch(nlev, batch, npts, first);
                first = false;
            }
    printf("\n],\"violations\":%d}\n", g_fail);
    if (g_fail) fprintf(stderr, "%d violations\n", g_fail);
    return g_fail ? 1 : 0;
}
