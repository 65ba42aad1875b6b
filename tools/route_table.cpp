// Prints the "Step route" table of DESIGN.md section 2 from psgd_plan::route / out_route: per caller,
// rank bucket, iterations per step and step parity the kernels one step launches. The plan flags
// are set to what psgd_geometry.cpp admits per rank bucket when every matrix fits (fin_ok: ranks
// 1-2; fin_proj: I = 2, ranks 1/2/4; oe_ok: rank 1, I >= 3; qfold_ok: ranks 2/4); a plan that
// misses one of them takes the row of the next bucket without it. No device is touched.
// build + run (from the repository root, after the library is built):
//   hipcc -std=c++17 -Iinclude -Ipowersgd_amd/csrc tools/route_table.cpp -Lpowersgd_amd/_lib -lpsgd \
//         -Wl,-rpath,$PWD/powersgd_amd/_lib -o /tmp/route_table && /tmp/route_table
#include <cstdio>
#include <string>

#include "psgd_plan.h"

namespace {

struct Caller {
    const char* name;
    bool world1, ipc, mix;  // aggregate_ctx's context; psgd_aggregate_ipc's; a mixed instance
};

std::string step_launches(psgd_plan& p, const Caller& who, int64_t step) {
    const MixArgs none{};
    StepCtx c;
    if (who.ipc) {
        c.fuse = p.rbucket == 1;
        c.raw_slot = 2;
        c.xgram = p.qfold_ok && p.iters == 2 && p.even(step, 0);
    }
    if (who.mix && who.world1) c.mix = &none;
    if (who.world1) c = world1_ctx(c);
    std::string s;
    for (int it = 0; it < p.iters; ++it) {
        const IterRoute r = p.route(step, it, c);
        if (r.orth == IterRoute::OrthLaunch) s += "orth ";
        if (r.orth == IterRoute::OrthChain) s += "orth_chain ";
        switch (r.pass) {
            case IterRoute::PassEven: s += "even reduce"; break;
            case IterRoute::PassOdd: s += "odd reduce"; break;
            case IterRoute::PassOddEven: s += "final_oe"; break;
            case IterRoute::PassFromOddEven: s += "reduce"; break;
            case IterRoute::PassFinal: s += std::string(r.proj ? "final_proj" : "final_odd") + (c.mix ? "_mix" : ""); break;
        }
        s += "; ";
    }
    const OutRoute o = p.out_route(step, who.world1 ? 1 : 2, who.world1 ? c : comm_out_ctx(who.mix ? &none : nullptr));
    if (o.kind == OutRoute::None) return s + "=> (none)";
    s += o.kind == OutRoute::Lowrank ? "=> lowrank" : "=> apply";
    return s + (o.inst == OutRoute::Plain ? (o.kind == OutRoute::Lowrank ? "_out" : "") : o.inst == OutRoute::Mix ? "_mix" : "_mix_w");
}

}  // namespace

int main() {
    const Caller callers[] = {{"psgd_aggregate", true, false, false},
                              {"building blocks, psgd_aggregate_comm", false, false, false},
                              {"psgd_aggregate_ipc", false, true, false},
                              {"psgd_aggregate_mixed", true, false, true},
                              {"psgd_aggregate_mixed_comm (W > 1)", false, false, true}};
    std::printf("| caller | rank bucket | I | step parity | launches (`;` ends an iteration, `=>` the output pass) |\n");
    std::printf("|---|---|---|---|---|\n");
    for (const Caller& who : callers)
        for (int R : {1, 2, 4, 8, 16}) {
            // mixed instances: rank buckets 1 / 2 / 4 and 16 / 32, not 8; the other callers' rows of
            // bucket 8 stand for 8-32
            if (who.mix ? R == 8 : R == 16) continue;
            for (int I = 1; I <= 4; ++I) {
                psgd_plan p;
                p.rbucket = R;
                p.iters = I;
                p.dtype = PSGD_F32;
                p.fin_ok = R <= 2;
                p.fin_proj = I == 2 && R <= 4;
                p.oe_ok = R == 1 && I >= 3;
                p.qfold_ok = R == 2 || R == 4;
                const std::string a = step_launches(p, who, 0), b = step_launches(p, who, 1);
                const char* rb = R == 16 ? "16-32" : R == 8 ? "8-32" : R == 1 ? "1" : R == 2 ? "2" : "4";
                if (a == b) {
                    std::printf("| %s | %s | %d | any | %s |\n", who.name, rb, I, a.c_str());
                } else {
                    std::printf("| %s | %s | %d | even | %s |\n", who.name, rb, I, a.c_str());
                    std::printf("| %s | %s | %d | odd | %s |\n", who.name, rb, I, b.c_str());
                }
            }
        }
    return 0;
}
