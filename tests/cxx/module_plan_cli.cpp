// module_plan_cli.cpp -- TEST-ONLY (tests/test_module_plan.py): the launch plans of csrc/module_plan.h on the CPU.  Host code only: built with
// the HIP compiler's host pass (the plan header needs dim3 and the transforms' constants) and run on a machine without a GPU.
//
// stdin: one query per line, "<stage> key=value ..." (missing keys are zero).  stdout: one line per query, "key=value ...".
//   mask          N noisy_first n_streams n_frames
//   bmask         N n_streams n_frames              (analyse_*, scan_*, synth_* launches)
//   mb_analyse    N n_arrays n_frames
//   mb_scan       nbins D n_arrays n_frames
//   mb_summary    n_arrays
//   tgcc          W8 nd n_arrays n_frames           (frames_*, gate_*, hook_* launches)
//   run_length    n_streams n_frames target lo hi
//   fpb           n_rows n_frames hi lo target
//   grid_for      n per
#include "../../mcarray_amd/csrc/module_plan.h"

#include <cstdio>
#include <iostream>
#include <map>
#include <sstream>
#include <string>

using namespace mca;

namespace {

typedef std::map<std::string, double> Query;
double get(const Query &q, const char *k) { auto it = q.find(k); return it == q.end() ? 0.0 : it->second; }
int geti(const Query &q, const char *k) { return (int)get(q, k); }

std::string dims(const std::string &name, dim3 d)
{
    char b[96];
    std::snprintf(b, sizeof b, " %s=%u,%u,%u", name.c_str(), d.x, d.y, d.z);
    return b;
}
// attr: what the one launcher decides from the plan's LDS (host_common.h)
std::string launch_text(const Launch &l, const std::string &pre = "")
{
    return dims(pre + "grid", l.grid) + dims(pre + "block", l.block) + " " + pre + "lds=" + std::to_string(l.lds) + " " + pre + "attr=" + (l.lds > 64 * 1024 ? "1" : "0");
}
const char *const MASK_FORM[] = {"1024", "2048", "gen"}, *const MB_FORM[] = {"1024", "512", "gen"};

}  // namespace

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string stage, kv;
        if (!(in >> stage)) continue;
        Query q;
        while (in >> kv) {
            const size_t eq = kv.find('=');
            if (eq == std::string::npos) { std::cerr << "bad token " << kv << "\n"; return 2; }
            q[kv.substr(0, eq)] = std::stod(kv.substr(eq + 1));
        }
        const int N = geti(q, "N"), n_streams = geti(q, "n_streams"), n_arrays = geti(q, "n_arrays"), n_frames = geti(q, "n_frames");
        if (stage == "mask") {
            const MaskStreamPlan p = plan_mask_stream(N, geti(q, "noisy_first") != 0, n_streams, n_frames);
            std::cout << "form=mask_" << MASK_FORM[p.form] << " ft=" << p.ft << " nthr=" << p.nthr << " per_cu=" << p.per_cu << launch_text(p.l) << "\n";
        } else if (stage == "bmask") {
            const BmaskPlan p = plan_bmask(N, n_streams, n_frames);
            std::cout << "form=bmask_" << MASK_FORM[p.form] << " ft=" << p.ft << " n_runs=" << p.n_runs << launch_text(p.analyse, "analyse_") << launch_text(p.scan, "scan_")
                      << launch_text(p.synth, "synth_") << "\n";
        } else if (stage == "mb_analyse") {
            const MbAnalysePlan p = plan_mb_analyse(N, n_arrays, n_frames);
            std::cout << "form=mb_" << MB_FORM[p.form] << " fpb=" << p.fpb << launch_text(p.l) << "\n";
        } else if (stage == "mb_scan") {
            const MbScanPlan p = plan_mb_scan(geti(q, "nbins"), geti(q, "D"), n_arrays, n_frames);
            std::cout << "chunk=" << p.chunk << launch_text(p.l) << "\n";
        } else if (stage == "mb_summary") std::cout << launch_text(plan_mb_summary(n_arrays)).substr(1) << "\n";
        else if (stage == "tgcc") {
            const int W8 = geti(q, "W8"), nd = geti(q, "nd");
            std::cout << launch_text(plan_tgcc_frames(W8, nd, n_arrays, n_frames), "frames_").substr(1) << launch_text(plan_tgcc_gate(n_arrays), "gate_")
                      << launch_text(plan_tgcc_hook(nd), "hook_") << "\n";
        } else if (stage == "run_length") std::cout << "len=" << run_length(n_streams, n_frames, (long long)get(q, "target"), geti(q, "lo"), geti(q, "hi")) << "\n";
        else if (stage == "fpb") std::cout << "len=" << frames_per_block(geti(q, "n_rows"), n_frames, geti(q, "hi"), geti(q, "lo"), (long long)get(q, "target")) << "\n";
        else if (stage == "grid_for") std::cout << dims("grid", grid_for((long long)get(q, "n"), geti(q, "per"))).substr(1) << "\n";
        else { std::cerr << "unknown stage " << stage << "\n"; return 2; }
    }
    return 0;
}
