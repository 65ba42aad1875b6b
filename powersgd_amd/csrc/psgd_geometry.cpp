// Tile geometry and segmentation of a plan: the work lists of every kernel for the current
// vector widths and buckets, their capacities, and the workspace carve (psgd_plan.h).
#include <cassert>

#include "psgd_plan.h"

namespace {

struct Geom {
    int lanes, nstrip, nchunk, chunk_rows;
    int64_t ntiles;
};

// Tile geometry of one matrix for a vector width (see psgd_stream.cuh).
Geom geometry(int64_t n, int64_t m, int r, int vec, int64_t tile_elems) {
    const int V = vec ? 4 : 1;
    const int64_t nq = (m + V - 1) / V;
    Geom g;
    g.lanes = int(std::min<int64_t>(64, pow2ceil(nq)));
    const int rows_pass = kWaves * (64 / g.lanes);
    g.nstrip = int((nq + g.lanes - 1) / g.lanes);
    int64_t cr = tile_elems / (int64_t(g.lanes) * V);
    // a small matrix must still spread over several workgroups (its tile is a serial chain)
    cr = std::min<int64_t>(cr, std::max<int64_t>(rows_pass, round_up((n + 7) / 8, rows_pass)));
    cr = std::max<int64_t>(cr, rows_pass);
    cr = round_up(cr, rows_pass);
    cr = std::min(cr, round_up(n, rows_pass));
    g.chunk_rows = int(cr);
    g.nchunk = int((n + cr - 1) / cr);
    g.ntiles = int64_t(g.nchunk) * g.nstrip;
    return g;
}

struct OddGeom {
    int sw, chunk_rows, nstrip, nchunk;
};

// MFMA odd-product tiles: strips of up to 256 columns (kOddSW, psgd_stream.cuh), chunks of
// 64 * g rows (4 waves x 16-row groups x g) sized to about tile_elems elements.
OddGeom odd_geometry(int64_t n, int64_t m, int64_t tile_elems) {
    OddGeom g;
    g.sw = int(std::min<int64_t>(256, round_up(m, 16)));
    const int64_t rows_pass = 16 * kWaves;
    int64_t groups = std::max<int64_t>(1, tile_elems / (rows_pass * g.sw));
    // a small matrix must still spread over several workgroups (as geometry())
    groups = std::min(groups, std::max<int64_t>(1, ((n + 7) / 8 + rows_pass - 1) / rows_pass));
    int64_t cr = std::min(groups * rows_pass, round_up(n, rows_pass));
    g.chunk_rows = int(cr);
    g.nstrip = int((m + g.sw - 1) / g.sw);
    g.nchunk = int((n + cr - 1) / cr);
    return g;
}

struct FinGeom {
    int T, S, rows;
    int64_t ntiles;
};

// Fused final odd pass (psgd_final.cuh): row groups of T threads (4 columns each, S
// segments), fin_rb(R) rows per group per batch, blocks of about fin_elems elements.
#ifndef PSGD_FIN_RB12
#define PSGD_FIN_RB12 1
#endif
int fin_rb(int R) { return R == 4 ? 1 : PSGD_FIN_RB12; }   // == FinRB<R>
#ifndef PSGD_FIN_NT4
#define PSGD_FIN_NT4 256  // == psgd_final.cuh
#endif
int fin_nt(int R) { return R == 4 ? PSGD_FIN_NT4 : 256; }  // == FinNT<R>
// scap = 0: the widest row group (T = min(threads, 4-column units rounded up to a power of
// two), fewest segments). scap > 0: the row group with the fewest idle lanes among
// S <= scap (ties: the narrower group — more rows per batch and, at T <= 64, a row sum
// within one wave instead of across waves through LDS); e.g. m = 576: T = 32, S = 5 (10 %
// idle) rather than T = 256, S = 1 (44 % idle).
FinGeom fin_geometry(int64_t n, int64_t m, int R, int64_t fin_elems, int scap = 0) {
    FinGeom g;
    const int nt = fin_nt(R), rb = fin_rb(R);
    const int64_t q4 = (m + 3) / 4;
    g.T = int(std::min<int64_t>(nt, pow2ceil(q4)));
    g.S = int((q4 + g.T - 1) / g.T);
    if (scap > 0) {
        int64_t best = int64_t(g.S) * g.T;
        for (int T = g.T / 2; T >= 4; T /= 2) {
            const int64_t S = (q4 + T - 1) / T;
            if (S > scap) break;
            if (S * T <= best) {
                best = S * T;
                g.T = T;
                g.S = int(S);
            }
        }
    }
    const int64_t batch = int64_t(nt / g.T) * rb;  // rows per workgroup batch
    int64_t rows = round_up(std::max<int64_t>(1, (fin_elems + m - 1) / m), batch);
    // a small matrix must still spread over several workgroups
    rows = std::min(rows, std::max(batch, round_up((n + 7) / 8, batch)));
    rows = std::min(rows, round_up(n, batch));
    // at most kFinRowsMax rows (a multiple of batch)
    rows = std::min(rows, std::max(batch, kFinRowsMax / batch * batch));
    g.rows = int(rows);
    g.ntiles = (n + rows - 1) / rows;
    return g;
}

}  // namespace

int psgd::fin_bucket(int s) { return s <= 2 ? 2 : s <= 3 ? 3 : s <= 5 ? 5 : s <= 12 ? 12 : 0; }

psgd_plan::Span psgd_plan::full_span() const {
    auto n = [](const auto& v) { return int32_t(v.size()); };
    return Span{{0, n(tiles)},    {0, n(tiles_ov)}, {0, n(tiles_om)}, {0, n(tiles_fin)}, {0, n(tiles_fin_kt)},
                {0, n(red_even)}, {0, n(red_odd)},  {0, n(units_p)},  {0, n(units_q)},
                {0, wg_seg.empty() ? 0 : n(wg_seg) - 1}, {0, ptot}, {0, qtot}};  // Span's member order
}

void psgd_plan::build_spans() {
    spans.clear();
    int32_t g0 = 0;
    for (size_t b = 0; b < bucket_gend.size(); ++b) {
        const int32_t g1 = bucket_gend[b];
        auto in = [&](int32_t mat) { const int32_t g = mats[mat].group; return g >= g0 && g < g1; };
        auto range = [&](const auto& v, auto key, int32_t (&r)[2]) {
            r[0] = int32_t(v.size());
            r[1] = 0;
            for (size_t i = 0; i < v.size(); ++i)
                if (key(v[i])) {
                    r[0] = std::min(r[0], int32_t(i));
                    r[1] = int32_t(i) + 1;
                }
            if (r[1] == 0) r[0] = 0;
        };
        Span sp{};
        auto tk = [&](const Tile& t) { return in(t.mat); };
        auto rk = [&](const RedItem& it) { return in(it.mat); };
        range(tiles, tk, sp.tiles);
        range(tiles_ov, tk, sp.ov);
        range(tiles_om, tk, sp.om);
        range(tiles_fin, tk, sp.fin);
        range(tiles_fin_kt, tk, sp.fin_kt);
        range(red_even, rk, sp.re);
        range(red_odd, rk, sp.ro);
        range(unit_group_p, [&](int32_t g) { return g >= g0 && g < g1; }, sp.up);
        range(unit_group_q, [&](int32_t g) { return g >= g0 && g < g1; }, sp.uq);
        sp.wg[0] = bucket_wg[2 * b];
        sp.wg[1] = bucket_wg[2 * b + 1];
        sp.p[0] = groups[g0].poff;
        sp.q[0] = groups[g0].qoff;
        sp.p[1] = g1 < int32_t(groups.size()) ? groups[g1].poff : ptot;
        sp.q[1] = g1 < int32_t(groups.size()) ? groups[g1].qoff : qtot;
        spans.push_back(sp);
        g0 = g1;
    }
}

void psgd_plan::set_f64_tiles() {
    f64_even.clear();
    f64_odd.clear();
    f64_apply.clear();
    f64_part_off.clear();
    f64_part = 0;
    vec_now = base_vec;
    red_even.clear();
    red_odd.clear();
    for (size_t i = 0; i < mats.size(); ++i) {
        MatDesc& d = mats[i];
        d.vec = 0;
        d.nstrip = int32_t((d.m + kF64Cols - 1) / kF64Cols);
        d.nchunk = int32_t((d.n + kF64Rows - 1) / kF64Rows);
        d.chunk_rows = int32_t(std::max<int64_t>(1, 16384 / d.m));  // apply: ~16k elements per tile
        for (int c = 0; c < d.nchunk; ++c)
            for (int st = 0; st < d.nstrip; ++st) f64_even.push_back(Tile{int32_t(i), st, c, 0});
        for (int64_t b = 0; b * kF64OddRows < d.n; ++b) f64_odd.push_back(Tile{int32_t(i), 0, int32_t(b), 0});
        for (int64_t b = 0; b * d.chunk_rows < d.n; ++b) f64_apply.push_back(Tile{int32_t(i), 0, int32_t(b), 0});
        f64_part_off.push_back(f64_part);
        f64_part += int64_t(d.nchunk) * kWaves * d.m * d.r;
        // k_f64_reduce: 64 consecutive Q elements per item (start only)
        for (int64_t s = 0; s < d.m * d.r; s += kRedElems)
            red_even.push_back(RedItem{int32_t(i), int32_t(s), 1, int32_t(std::min<int64_t>(kRedElems, d.m * d.r - s)), 0, 0, 0});
    }
}

// Wide plans (psgd_wide.hip). A product workgroup owns kWideOut out-factor rows (matrix columns
// for the even product, matrix rows for the odd one) and sums over one chunk of the other
// dimension; a matrix is cut into about 1024 / (its out blocks) chunks of at least 512, so a
// plan of one large matrix still fills the chip and the partials stay under a quarter of the
// gradient traffic at rank 128. Partials [chunks][out rows][r] are summed in chunk order.
void psgd_plan::set_wide_tiles() {
    wide_even.clear();
    wide_odd.clear();
    wide_apply.clear();
    wide_part = 0;
    vec_now = base_vec;
    red_even.clear();
    red_odd.clear();
    // orthonormalisation: row blocks of every rank > 1 panel (rank-1 units have no Gram)
    wide_slots = 0;
    for (int side = 0; side < 2; ++side) {
        const DevList<OrthUnit>& units = side ? units_q : units_p;
        DevList<Tile>& items = side ? wide_gq : wide_gp;
        DevList<int32_t>& slot0 = side ? wide_slot_q : wide_slot_p;
        items.clear();
        slot0.clear();
        int32_t slot = 0;
        for (size_t ui = 0; ui < units.size(); ++ui) {
            slot0.push_back(slot);
            if (units[ui].r == 1) continue;
            for (int64_t b = 0; b * kWideGramRows < units[ui].k; ++b) items.push_back(Tile{int32_t(ui), int32_t(b), slot++, 0});
        }
        wide_slots = std::max<int64_t>(wide_slots, slot);
    }
    auto chunk_of = [](int64_t out_len, int64_t sum_len) {
        const int64_t nout = (out_len + kWideOut - 1) / kWideOut;
        const int64_t want = std::max<int64_t>(1, 1024 / nout);
        const int64_t nch = std::max<int64_t>(1, std::min(want, (sum_len + 511) / 512));
        return round_up((sum_len + nch - 1) / nch, kWideStep);
    };
    for (size_t i = 0; i < mats.size(); ++i) {
        MatDesc& d = mats[i];
        d.vec = 0;
        // even: out = columns, summed over row chunks
        d.nstrip = int32_t((d.m + kWideOut - 1) / kWideOut);
        d.chunk_rows = int32_t(chunk_of(d.m, d.n));
        d.nchunk = int32_t((d.n + d.chunk_rows - 1) / d.chunk_rows);
        d.part_even = wide_part;
        wide_part += int64_t(d.nchunk) * d.m * d.r;
        // odd: out = rows, summed over column strips
        d.odd_mfma = 1;
        d.odd_chunk_rows = kWideOut;
        d.odd_sw = int32_t(chunk_of(d.n, d.m));
        d.odd_nstrip = int32_t((d.m + d.odd_sw - 1) / d.odd_sw);
        d.part_odd = wide_part;
        wide_part += int64_t(d.odd_nstrip) * d.n * d.r;
        const int32_t nrb = int32_t((d.n + kWideOut - 1) / kWideOut);
        for (int c = 0; c < d.nchunk; ++c)
            for (int st = 0; st < d.nstrip; ++st) wide_even.push_back(Tile{int32_t(i), st, c, d.tensor});
        for (int b = 0; b < nrb; ++b)
            for (int st = 0; st < d.odd_nstrip; ++st) wide_odd.push_back(Tile{int32_t(i), st, b, d.tensor});
        for (int b = 0; b < nrb; ++b)
            for (int64_t st = 0; st * kWideApplyCols < d.m; ++st)
                wide_apply.push_back(Tile{int32_t(i), int32_t(st), b, d.tensor});
        // k_wide_reduce: kRedItem consecutive factor elements per item
        for (int64_t s = 0; s < d.m * d.r; s += kRedItem)
            red_even.push_back(RedItem{int32_t(i), int32_t(s), 1, int32_t(std::min<int64_t>(kRedItem, d.m * d.r - s)), 0, 0,
                                       d.nchunk});
        for (int64_t s = 0; s < d.n * d.r; s += kRedItem)
            red_odd.push_back(RedItem{int32_t(i), int32_t(s), 1, int32_t(std::min<int64_t>(kRedItem, d.n * d.r - s)), 0, 0,
                                      d.odd_nstrip});
    }
}

// Even-product segmentation (k_even) and every reduction item list, for the current strip
// geometry and buckets. Per bucket (or the whole plan), the gradient elements of its
// matrices (walked matrix -> strip -> row) are cut into nwg equal ranges, one per workgroup;
// a segment ends at a strip end or at a workgroup's range end. Partials: per strip, its
// segments' [W x r] slabs in row order (W = lanes x V strip columns).
void psgd_plan::build_reduction() {
    segs.clear();
    wg_seg.clear();
    bucket_wg.clear();
    red_even.clear();
    red_odd.clear();
    red_even_b.assign(mats.size(), 0);
    red_even_e.assign(mats.size(), 0);
    grng_even.assign(2 * groups.size(), 0);
    grng_odd.assign(2 * groups.size(), 0);
    grng_ss0.assign(2 * groups.size(), 0);
    std::vector<int32_t> ends = bucket_gend;
    if (ends.empty()) ends.push_back(int32_t(groups.size()));
    // pass 1: segments per bucket
    std::vector<std::vector<int32_t>> nseg(mats.size());  // per matrix, per strip: segment count
    for (size_t i = 0; i < mats.size(); ++i) nseg[i].assign(size_t(mats[i].nstrip), 0);
    size_t mi = 0;
    for (int32_t g1 : ends) {
        size_t m0 = mi;
        while (mi < mats.size() && mats[mi].group < g1) ++mi;
        int64_t total = 0;
        for (size_t i = m0; i < mi; ++i) total += mats[i].n * mats[i].m;
        int64_t nwg_launch = std::max<int64_t>(
            1, std::min<int64_t>(int64_t(even_wpc) * kCUs, (total + even_min - 1) / std::max<int64_t>(even_min, 1)));
        const int64_t nwg = nwg_launch;  // ranges cut below, one per workgroup
        bucket_wg.push_back(int32_t(wg_seg.size()));
        int64_t cum = 0, w = 0;
        wg_seg.push_back(int32_t(segs.size()));
        auto make = [&](size_t i, int s, int64_t r0, int64_t r1) {
            const MatDesc& d = mats[i];
            Seg sg{};
            sg.m = d.m;
            sg.poff = d.poff;
            sg.qoff = d.qoff;
            sg.row0 = int32_t(r0);
            sg.row1 = int32_t(r1);
            sg.strip = s;
            sg.tensor = d.tensor;
            sg.ss = -1;
            sg.r = d.r;
            sg.lanes = d.lanes;
            sg.vec = d.vec;
            // full-width strips of an r == R matrix take k_even's scalar-row fast path
            if (d.vec && d.lanes == 64 && d.r == rbucket && rbucket <= 8) sg.vec = 2;
            sg.part = int64_t(i);  // matrix index for now (pass 2)
            segs.push_back(sg);
            ++nseg[i][size_t(s)];
        };
        // Cost model (round 4, the per-workgroup stamps of profiles/r04/b): a workgroup's
        // time is its gradient loads plus a fixed cost per segment (descriptor loads, a
        // fresh load batch, the epilogue: ~1.5-2 us, i.e. even_segc elements at one
        // workgroup's streaming rate), and a scalar-column strip (V = 1: 256 B per wave
        // load instead of 1 KB) costs 4x per element. Equal COST ranges instead of equal
        // bytes: the first workgroup used to take the five narrow segments of conv1 and the
        // first 64-row matrices and finish last (22 us against p99 19 us).
        const int64_t segc = even_segc;
        // (ranks 16 / 32: m % 4 == 0 strips stream 16-byte row quads on the matrix cores,
        // even_seg_mfma, at the vector rate)
        auto rowc = [&](const MatDesc& d, int64_t cols) {
            return cols * ((d.vec || (rbucket >= 16 && d.m % 4 == 0)) ? 1 : 4);
        };
        int64_t totw = nwg * segc;
        for (size_t i = m0; i < mi; ++i) {
            const MatDesc& d = mats[i];
            const int64_t W = int64_t(d.lanes) * (d.vec ? 4 : 1);
            for (int s = 0; s < d.nstrip; ++s) totw += d.n * rowc(d, std::min<int64_t>(W, d.m - s * W)) + segc;
        }
        // (a dispatch-order skew, more cost to low block indices, was measured and does not
        // help: the late blocks finish late whatever their share, profiles/r04/e)
        auto wbound = [&](int64_t ww) { return ww + 1 >= nwg ? totw : (ww + 1) * totw / nwg; };
        for (size_t i = m0; i < mi; ++i) {
            const MatDesc& d = mats[i];
            const int64_t W = int64_t(d.lanes) * (d.vec ? 4 : 1);
            for (int s = 0; s < d.nstrip; ++s) {
                const int64_t cols = std::min<int64_t>(W, d.m - s * W);
                const int64_t rc = rowc(d, cols);
                // k_even addresses a segment with 32-bit offsets: at most 2^30 bytes each
                const int64_t es = dtype == PSGD_BF16 ? 2 : 4;
                const int64_t seg_max = std::max<int64_t>(1, ((int64_t(1) << 30) / (d.m * es)) - 64);
                int64_t r0 = 0;
                while (r0 < d.n) {
                    int64_t take = std::min(d.n - r0, seg_max);
                    if (w < nwg - 1) {
                        // rows to this range's end, after paying the segment's fixed cost
                        const int64_t fit = (wbound(w) - cum - segc + rc / 2) / rc;
                        if (fit <= 0) {
                            ++w;
                            wg_seg.push_back(int32_t(segs.size()));
                            continue;
                        }
                        take = std::min(take, fit);
                    }
                    make(i, s, r0, r0 + take);
                    cum += segc + take * rc;
                    r0 += take;
                    if (w < nwg - 1 && cum >= wbound(w)) {  // this range is full
                        ++w;
                        wg_seg.push_back(int32_t(segs.size()));
                    }
                }
            }
        }
        while (int64_t(wg_seg.size()) - bucket_wg.back() < nwg + 1) wg_seg.push_back(int32_t(segs.size()));
        bucket_wg.push_back(int32_t(wg_seg.size()) - 1);
    }
    // wg_seg holds nwg + 1 bounds per bucket; the buckets' ranges are concatenated so that
    // workgroup w of the whole launch reads wg_seg[w], wg_seg[w + 1]: drop each bucket's
    // closing bound except the last
    {
        std::vector<int32_t> flat;
        std::vector<int32_t> bw;
        for (size_t b = 0; b * 2 < bucket_wg.size(); ++b) {
            const int32_t lo = bucket_wg[2 * b], hi = bucket_wg[2 * b + 1];
            bw.push_back(int32_t(flat.size()));
            for (int32_t k = lo; k < hi; ++k) flat.push_back(wg_seg[size_t(k)]);
            bw.push_back(int32_t(flat.size()));
        }
        flat.push_back(int32_t(segs.size()));
        wg_seg.swap(flat);
        bucket_wg.swap(bw);
    }
    // pass 2: partial slabs (per matrix, per strip, segments in row order) and ss slots
    std::vector<std::vector<int64_t>> base(mats.size());
    int64_t off = (part_odd_floats + 3) & ~int64_t(3);
    for (size_t i = 0; i < mats.size(); ++i) {
        const MatDesc& d = mats[i];
        const int64_t W = int64_t(d.lanes) * (d.vec ? 4 : 1);
        base[i].assign(size_t(d.nstrip), 0);
        for (int s = 0; s < d.nstrip; ++s) {
            base[i][size_t(s)] = off;
            off += (int64_t(nseg[i][size_t(s)]) * W * d.r + 3) & ~int64_t(3);
        }
    }
    std::vector<std::vector<int32_t>> kseg(mats.size());
    for (size_t i = 0; i < mats.size(); ++i) kseg[i].assign(size_t(mats[i].nstrip), 0);
    int32_t ss = 0;
    // strip-0 segments get consecutive slots in matrix order (a group's slots contiguous)
    std::vector<std::vector<int32_t>> s0(mats.size());
    for (Seg& sg : segs) {
        const size_t i = size_t(sg.part);
        const MatDesc& d = mats[i];
        const int64_t W = int64_t(d.lanes) * (d.vec ? 4 : 1);
        const int32_t k = kseg[i][size_t(sg.strip)]++;
        sg.part = base[i][size_t(sg.strip)] + int64_t(k) * W * d.r;
        if (sg.strip == 0) s0[i].push_back(int32_t(&sg - segs.data()));
    }
    for (size_t i = 0; i < mats.size(); ++i) {
        const int g = mats[i].group;
        if (i == 0 || mats[i - 1].group != g) grng_ss0[2 * g] = ss;
        for (int32_t si : s0[i]) segs[size_t(si)].ss = ss++;
        grng_ss0[2 * g + 1] = ss;
    }
    // reduction items: even ones per strip (its segments' partials), odd ones per matrix
    for (size_t i = 0; i < mats.size(); ++i) {
        const MatDesc& d = mats[i];
        const int g = d.group;
        const bool first = i == 0 || mats[i - 1].group != g;
        if (first) {
            grng_even[2 * g] = int32_t(red_even.size());
            grng_odd[2 * g] = int32_t(red_odd.size());
        }
        const int64_t W = int64_t(d.lanes) * (d.vec ? 4 : 1);
        red_even_b[i] = int32_t(red_even.size());
        for (int s = 0; s < d.nstrip; ++s) {
            const int np = nseg[i][size_t(s)];
            const int pe = np > kRedWide ? 1 : 4;
            const int64_t e0 = s * W * d.r, e1 = std::min<int64_t>((s + 1) * W, d.m) * d.r;
            for (int64_t e = e0; e < e1; e += 64 * pe)
                red_even.push_back(RedItem{int32_t(i), int32_t(e), pe, int32_t(std::min<int64_t>(64 * pe, e1 - e)),
                                           base[i][size_t(s)] + (e - e0), int32_t(W * d.r), np});
        }
        red_even_e[i] = int32_t(red_even.size());
        const int npo = d.odd_nstrip;
        const int po = npo > kRedWide ? 1 : 4;
        for (int64_t e = 0; e < d.n * d.r; e += 64 * po)
            red_odd.push_back(RedItem{int32_t(i), int32_t(e), po, int32_t(std::min<int64_t>(64 * po, d.n * d.r - e)),
                                      d.part_odd + e, int32_t(d.n * d.r), npo});
        grng_even[2 * g + 1] = int32_t(red_even.size());
        grng_odd[2 * g + 1] = int32_t(red_odd.size());
    }
    mrng_even.clear();
    for (size_t i = 0; i < mats.size(); ++i) {
        mrng_even.push_back(red_even_b[i]);
        mrng_even.push_back(red_even_e[i]);
    }
    // folded orthonormalisation: per Q unit (one matrix each) its even item range
    uitems.clear();
    if (qfold_ok) {
        for (const OrthUnit& u : units_q)
            for (size_t i = 0; i < mats.size(); ++i)
                if (mats[i].qoff == u.off) {
                    uitems.push_back(red_even_b[i]);
                    uitems.push_back(red_even_e[i]);
                }
    }
}

void psgd_plan::set_vec(const std::vector<int>& vec) {
    vec_now = vec;
    tiles.clear();
    tiles_ov.clear();
    tiles_om.clear();
    tiles_fin.clear();
    tiles_fin_kt.clear();
    int64_t podd = 0;
    for (size_t i = 0; i < mats.size(); ++i) {
        MatDesc& d = mats[i];
        const Geom g = geometry(d.n, d.m, d.r, vec[i], tile_elems);
        d.vec = vec[i];
        d.lanes = g.lanes;
        d.nstrip = g.nstrip;
        d.nchunk = g.nchunk;
        d.chunk_rows = g.chunk_rows;
        const OddGeom og = odd_geometry(d.n, d.m, tile_elems);
        // the MFMA kernel addresses a tile through a buffer descriptor (< 2^31 bytes)
        const int64_t span = ((int64_t(og.chunk_rows) - 1) * d.m + og.sw) * (dtype == PSGD_BF16 ? 2 : 4);
        // r <= 4: every odd tile stays in ONE k_product_odd launch (row layout with a
        // reduce-scatter on full-width strips, lane sums on narrow ones); the MFMA kernel
        // pays for itself only for wider factors (16 output columns per instruction)
        const bool valu = d.r <= 4;
        d.odd_mfma = (!valu && d.r <= 32 && span < (int64_t(1) << 31)) ? 1 : 0;
        for (int c = 0; c < g.nchunk; ++c)
            for (int s = 0; s < g.nstrip; ++s) {
                tiles.push_back(Tile{int32_t(i), s, c, d.tensor});
                if (!d.odd_mfma) tiles_ov.push_back(Tile{int32_t(i), s, c, d.tensor});
            }
        if (d.odd_mfma) {
            d.odd_sw = og.sw;
            d.odd_chunk_rows = og.chunk_rows;
            d.odd_nstrip = og.nstrip;
            for (int c = 0; c < og.nchunk; ++c)
                for (int s = 0; s < og.nstrip; ++s) tiles_om.push_back(Tile{int32_t(i), s, c, d.tensor});
        } else {
            d.odd_sw = d.odd_chunk_rows = 0;
            d.odd_nstrip = g.nstrip;
        }
        // odd partials [odd strips][n][r], 16-byte aligned slabs (k_reduce's vector loads)
        d.part_odd = podd = (podd + 3) & ~int64_t(3);
        podd += int64_t(d.odd_nstrip) * d.n * d.r;
        d.part_even = 0;
    }
    part_odd_floats = podd;
    fin_ok = false;
    fin_proj = false;
    // buffer descriptors address one matrix: keep each below 2^31 bytes
    bool small = true;
    for (const MatDesc& d : mats) small = small && d.n * d.m * (dtype == PSGD_BF16 ? 2 : 4) < (int64_t(1) << 31);
    int smax = 0;
    for (const MatDesc& d : mats) smax = std::max(smax, fin_geometry(d.n, d.m, rbucket, 0).S);
    // >= 2 waves per SIMD resident (the register arrays scale with S * 4 * r)
    auto fits = [&](int nres) {
        int waves = 0;
        FinalArgs none{};
        return fin_bucket(smax) > 0 &&
               launch_final_odd(dtype, rbucket, nres, fin_bucket(smax), none, 0, nullptr, &waves) == hipSuccess &&
               waves >= 2;
    };
    // The fused forms (fuse_final_on): K-term at ranks 1-2, projection at ranks 1/2/4. The rank-4
    // K-term form (two register panels: 253 VGPRs, one 512-thread workgroup per CU,
    // profiles/r04/regs_final_f32.txt) measured 0.152 vs 0.119 ms for the unfused world-size > 1
    // step (profiles/r03/k) and is not built
    if (fuse_final_on && small && rbucket <= 2) fin_ok = fits(iters - 1);
    // the K-term form exists for ranks 1-2 only (dispatch_final_k<4> refuses any K-term nres)
    assert(!fin_ok || rbucket <= 2);
    // Projection form (psgd_final.cuh): two power iterations at world size 1, ranks 2 and 4,
    // the last iteration's in-factor orthonormalised by Cholesky-QR (which leaves R').
    // Same register-panel geometry as the K-term form, so both can share the tile list.
    // Rank 1 (the joint group norm folded into the kernels, psgd_aggregate): the same form with
    // the per-matrix correction of psgd_final.cuh; it needs the folded norm's sums of squares.
    if (fuse_final_on && fin_proj_on && small && iters == 2 &&
        (((rbucket == 2 || rbucket == 4) && orth_chol) || rbucket == 1))
        fin_proj = fits(kFinProj);
    fin_smax = 0;
    if (fin_ok || fin_proj) {
        // segments per row up to the kernel bucket the widest groups already need
        // (at most 5: the exact-S bodies), for fewer idle lanes
        const int scap = std::min(fin_bucket(smax), 5);
        // row blocks: the projection form's fin_elems; the K-term form's fin_elems_kt (its own
        // list only when both forms exist and the sizes differ; fin_rows_kt = fin_rows else)
        const int64_t fe = fin_proj ? fin_elems : fin_elems_kt;
        const bool two = fin_proj && fin_ok && fin_elems_kt != fin_elems;
        for (size_t i = 0; i < mats.size(); ++i) {
            MatDesc& d = mats[i];
            const FinGeom fg = fin_geometry(d.n, d.m, rbucket, fe, scap);
            d.fin_T = fg.T;
            d.fin_S = fg.S;
            d.fin_rows = fg.rows;
            d.fin_rows_kt = fg.rows;
            fin_smax = std::max(fin_smax, fg.S);
            for (int64_t b = 0; b < fg.ntiles; ++b) tiles_fin.push_back(Tile{int32_t(i), 0, int32_t(b), d.tensor});
            if (two) {
                const FinGeom fk = fin_geometry(d.n, d.m, rbucket, fin_elems_kt, scap);
                d.fin_rows_kt = fk.rows;
                for (int64_t b = 0; b < fk.ntiles; ++b)
                    tiles_fin_kt.push_back(Tile{int32_t(i), 0, int32_t(b), d.tensor});
            }
        }
    }
    build_oe();
    build_reduction();
    fill_seam_descriptors();
    if (!bucket_gend.empty()) build_spans();
}

// What the rank-1 prologue of the fused final passes used to reach through MatDesc and the
// range tables, copied beside each row block: its group's and its matrix's item ranges.
void psgd_plan::fill_seam_descriptors() {
    for (DevList<FinRng>* l : {&rng_fin, &rng_fin_kt, &rng_oe}) l->clear();
    if (!seam_on()) return;
    auto pair_of = [](const std::vector<int32_t>& tab, size_t i, int32_t (&o)[2]) {
        o[0] = 2 * i + 1 < tab.size() ? tab[2 * i] : 0;
        o[1] = 2 * i + 1 < tab.size() ? tab[2 * i + 1] : 0;
    };
    auto blocks = [&](const DevList<Tile>& tl, DevList<FinRng>& out) {
        for (const Tile& t : tl) {
            FinRng f{};
            const size_t g = size_t(mats[size_t(t.mat)].group);
            pair_of(grng_even, g, f.g[0]);
            pair_of(grng_oe_items, g, f.g[1]);
            int32_t mr[2];
            pair_of(mrng_even, size_t(t.mat), mr);
            f.mb = mr[0];
            f.me = mr[1];
            out.push_back(f);
        }
    };
    blocks(tiles_fin, rng_fin);
    blocks(tiles_fin_kt, rng_fin_kt);
    blocks(tiles_oe, rng_oe);
}

void psgd_plan::build_oe() {
    oe_ok = false;
    red_oe.clear();
    tiles_oe.clear();
    grng_oe.assign(2 * groups.size(), 0);
    grng_oe_items.assign(2 * groups.size(), 0);
    oe_part_floats = 0;
    oe_blocks = 0;
    if (!fin_ok || rbucket != 1 || iters < 3 || f64() || !oe_on) return;
    int waves = 0;
    FinalArgs none{};
    if (launch_final_oe(dtype, iters - 2, fin_bucket(fin_smax), none, 0, nullptr, &waves) != hipSuccess || waves < 2)
        return;
    for (size_t i = 0; i < mats.size(); ++i) {
        MatDesc& d = mats[i];
        const int g = d.group;
        const bool first = i == 0 || mats[i - 1].group != g;
        if (first) {
            grng_oe[2 * g] = oe_blocks;
            grng_oe_items[2 * g] = int32_t(red_oe.size());
        }
        // one K-term row block per odd-even block (2 / 4 / 8 blocks merged: fewer partials
        // for the reduction but a slower pass, cfg5 0.0322 / 0.0333 / 0.041 against 0.0307 ms,
        // profiles/r05)
        d.oe_rows = int32_t(std::min<int64_t>(d.n, int64_t(d.fin_rows_kt)));
        const int32_t nb = int32_t((d.n + d.oe_rows - 1) / d.oe_rows);
        for (int32_t b = 0; b < nb; ++b) tiles_oe.push_back(Tile{int32_t(i), 0, b, d.tensor});
        d.oe_blk0 = oe_blocks;
        d.oe_part = oe_part_floats;
        oe_blocks += nb;
        oe_part_floats += int64_t(nb) * d.m;  // rank 1: [m] per block
        const int pe = nb > kRedWide ? 1 : 4;
        for (int64_t e = 0; e < d.m; e += 64 * pe)
            red_oe.push_back(RedItem{int32_t(i), int32_t(e), pe, int32_t(std::min<int64_t>(64 * pe, d.m - e)),
                                     d.oe_part + e, int32_t(d.m), nb});
        grng_oe[2 * g + 1] = oe_blocks;
        grng_oe_items[2 * g + 1] = int32_t(red_oe.size());
    }
    oe_ok = true;
}

// Capacities of every list set_vec may build (either vector width, up to kMaxBuckets buckets):
// tiles, segments, reduction items, partial slabs; then the first tiling and the workspace
// carve. The carve order, sizes and 256-byte alignment fix every device address.
void psgd_plan::layout(int num_tensors) {
    int64_t total = 0, strips_max = 0, strip_elems = 0, red_even_cap = 0, red_odd_cap = 0, part_odd_cap = 0, wr_max = 0;
    int64_t tiles_cap = 0, tiles_om_cap = 0, tiles_fin_cap = 0, tiles_fin_kt_cap = 0;
    for (size_t i = 0; i < mats.size(); ++i) {
        const MatDesc& md = mats[i];
        total += md.n * md.m;
        const OddGeom og = odd_geometry(md.n, md.m, tile_elems);
        int64_t ns = 0, se = 0, re = 0, po = og.nstrip;
        for (int v : {base_vec[i], 0}) {
            const Geom g = geometry(md.n, md.m, md.r, v, tile_elems);
            const int64_t W = int64_t(g.lanes) * (v ? 4 : 1);
            ns = std::max<int64_t>(ns, g.nstrip);
            se = std::max<int64_t>(se, g.nstrip * (W * md.r + 3));
            re = std::max<int64_t>(re, (md.m * md.r + 63) / 64 + g.nstrip);
            po = std::max<int64_t>(po, g.nstrip);
            wr_max = std::max<int64_t>(wr_max, W * md.r + 3);
        }
        tiles_cap += std::max(geometry(md.n, md.m, md.r, base_vec[i], tile_elems).ntiles,
                              geometry(md.n, md.m, md.r, 0, tile_elems).ntiles);
        tiles_om_cap += int64_t(og.nstrip) * og.nchunk;
        int64_t cap = 0, cap_kt = 0;
        for (int sc = 0; sc <= 5; ++sc) {  // any segment cap set_vec may pick
            cap_kt = std::max(cap_kt, fin_geometry(md.n, md.m, rbucket, fin_elems_kt, sc).ntiles);
            cap = std::max(cap, fin_geometry(md.n, md.m, rbucket, fin_elems, sc).ntiles);
        }
        tiles_fin_cap += std::max(cap, cap_kt);
        tiles_fin_kt_cap += cap_kt;
        strips_max += ns;
        strip_elems += se;
        red_even_cap += re;
        red_odd_cap += (md.n * md.r + 63) / 64;
        part_odd_cap += po * md.n * md.r + 3;
    }
    const int64_t nb = std::min<int64_t>(kMaxBuckets, int64_t(groups.size()));
    const int64_t wg = std::min<int64_t>(int64_t(even_wpc) * kCUs, total / even_min + 1);
    // segments beyond one per strip: one per workgroup boundary (strip walk), up to two per
    // workgroup (row blocks across strips, ragged strips)
    const int64_t extra = 2 * nb * wg;
    const int64_t segs_cap = strips_max + extra;
    ss0_cap = int64_t(mats.size()) + extra;
    const int64_t part_cap = part_odd_cap + 4 + strip_elems + extra * wr_max;
    if (f64()) {
        set_f64_tiles();  // fp64: its own kernels and tiles (psgd_f64.hip), no fused forms
        red_even_cap = std::max<int64_t>(red_even_cap, int64_t(red_even.size()));
    } else if (wide()) {
        set_wide_tiles();  // ranks 33-128: their own kernels and tiles (psgd_wide.hip), no fused forms
        red_even_cap = std::max<int64_t>(red_even_cap, int64_t(red_even.size()));
        red_odd_cap = std::max<int64_t>(red_odd_cap, int64_t(red_odd.size()));
    } else {
        set_vec(base_vec);
    }
    for (const MatDesc& md : mats) {
        munits_p.push_back(OrthUnit{md.poff, md.n, md.r, 1});
        munits_q.push_back(OrthUnit{md.qoff, md.m, md.r, 1});
    }

    size_t off = 0;
    auto scratch = [&](size_t bytes) {
        const size_t o = off;
        off = align256(off + bytes);
        return o;
    };
    auto atleast1 = [](int64_t x) { return size_t(std::max<int64_t>(x, 1)); };
    const size_t grng_cap = atleast1(2 * int64_t(groups.size()));
    o_ptrs = scratch(TableCache::bytes(size_t(num_tensors)));
    mats.carve(off, mats.size());
    tiles.carve(off, size_t(tiles_cap));
    tiles_ov.carve(off, size_t(tiles_cap));
    tiles_om.carve(off, atleast1(tiles_om_cap));
    tiles_fin.carve(off, atleast1(tiles_fin_cap));
    tiles_fin_kt.carve(off, atleast1(tiles_fin_kt_cap));
    segs.carve(off, atleast1(segs_cap));
    wg_seg.carve(off, size_t(kMaxBuckets) * kEvenWgMax + 1);
    red_even.carve(off, atleast1(red_even_cap));
    red_odd.carve(off, atleast1(red_odd_cap));
    units_p.carve(off, units_p.size());
    units_q.carve(off, units_q.size());
    munits_p.carve(off, munits_p.size());
    munits_q.carve(off, munits_q.size());
    ipc_peer.carve(off, size_t(kMaxRanks));
    ipc_nonces.carve(off, size_t(kMaxRanks));
    o_rq = scratch(atleast1(fmax) * sizeof(float));
    o_rdst = scratch(TableCache::bytes(size_t(num_tensors)));
    o_odst = scratch(TableCache::bytes(size_t(num_tensors)));
    grng_even.carve(off, grng_cap);
    grng_odd.carve(off, grng_cap);
    mrng_even.carve(off, atleast1(2 * int64_t(mats.size())));
    ss_stride = size_t(std::max<int64_t>({red_even_cap, red_odd_cap, int64_t(red_oe.size())}));
    if (oe_ok) {  // the odd-even pass's layout (geometry-independent: fixed at create)
        o_oe_part = scratch(size_t(oe_part_floats) * sizeof(float));
        tiles_oe.carve(off, atleast1(int64_t(tiles_oe.size())));
        o_oe_ss = scratch(atleast1(oe_blocks) * sizeof(float));
        red_oe.carve(off, atleast1(int64_t(red_oe.size())));
        grng_oe.carve(off, grng_cap);
        grng_oe_items.carve(off, grng_cap);
    }
    o_ss = scratch(2 * std::max<size_t>(ss_stride, 1) * sizeof(float));
    o_ss0 = scratch(atleast1(ss0_cap) * sizeof(float));
    grng_ss0.carve(off, grng_cap);
    o_hist = scratch(size_t(3) * iters * size_t(fmax) * (f64() ? sizeof(double) : sizeof(float)));
    f64_even.carve(off, atleast1(int64_t(f64_even.size())));
    f64_odd.carve(off, atleast1(int64_t(f64_odd.size())));
    f64_apply.carve(off, atleast1(int64_t(f64_apply.size())));
    f64_part_off.carve(off, atleast1(int64_t(f64_part_off.size())));
    o_f64_part = scratch(atleast1(f64_part) * sizeof(double));
    o_part = scratch(wide() ? 256 : size_t(part_cap) * sizeof(float));  // wide plans: o_wide_part
    if (qfold_ok) {
        o_gram = scratch(size_t(red_even_cap) * kGramStride * sizeof(double));
        uitems.carve(off, 2 * units_q.size());
    }
    if (seam_on()) {  // rank-1 plans: the FinRng lists (other plans' carve does not move)
        rng_fin.carve(off, atleast1(tiles_fin_cap));
        rng_fin_kt.carve(off, atleast1(tiles_fin_kt_cap));
        if (oe_ok) rng_oe.carve(off, atleast1(int64_t(tiles_oe.size())));
    }
    if (wide()) {  // behind everything else: the other plans' carve does not move
        wide_even.carve(off, atleast1(int64_t(wide_even.size())));
        wide_odd.carve(off, atleast1(int64_t(wide_odd.size())));
        wide_apply.carve(off, atleast1(int64_t(wide_apply.size())));
        o_wide_part = scratch(atleast1(wide_part) * sizeof(float));
        wide_gp.carve(off, atleast1(int64_t(wide_gp.size())));
        wide_gq.carve(off, atleast1(int64_t(wide_gq.size())));
        wide_slot_p.carve(off, atleast1(int64_t(wide_slot_p.size())));
        wide_slot_q.carve(off, atleast1(int64_t(wide_slot_q.size())));
        const size_t rr = size_t(rbucket) * rbucket, nu = std::max(units_p.size(), units_q.size());
        o_wide_gram = scratch(atleast1(wide_slots) * rr * sizeof(double));
        o_wide_m = scratch(nu * rr * sizeof(double));
        o_wide_sg = scratch(nu * size_t(rbucket) * sizeof(double));
        o_wide_ok = scratch(nu * sizeof(int32_t));
    }
    ws_bytes = off;
}

int psgd_plan::upload_tiles() const {
    if (int st = upload_all(ws, mats, tiles, tiles_ov, tiles_om, tiles_fin, tiles_fin_kt, segs, wg_seg, red_even,
                            red_odd, grng_even, grng_odd, grng_ss0, mrng_even, uitems))
        return st;
    if (seam_on())
        if (int st = upload_all(ws, rng_fin, rng_fin_kt)) return st;
    // (without the odd-even pass its lists are not carved)
    if (oe_ok && seam_on())
        if (int st = upload_all(ws, rng_oe)) return st;
    return oe_ok ? upload_all(ws, tiles_oe, red_oe, grng_oe, grng_oe_items) : PSGD_OK;
}
