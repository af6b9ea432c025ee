// mvdr_plan_cli.cpp -- TEST-ONLY (tests/test_mvdr_plan.py): the launch plans of csrc/mvdr_plan.h on the CPU.  Host code only: built with
// the HIP compiler's host pass (the plan header needs dim3 and the transforms' constants) and run on a machine without a GPU.
//
// stdin: one query per line, "<stage> key=value ...": the keys N and M of the context (K, H, tri follow) and the arguments of the stage's
// plan function (missing keys are zero).  stdout: one line per query, "key=value ...".
//   analyse       n_streams n_frames
//   solve_split   n_streams n_loop
//   solve_choice  rtf n_sources null_gain update masked pf_on      (have: mvdr_solve_choice_row)
//   rtf           n_streams n_sources n_frames cap_cells
//   estmask       n_streams n_frames
//   postfilter    n_streams n_sources
//   synth         n_streams n_sources n_frames
//   spectrum      bin_lo bin_hi Dpad n_streams
//   tracks        bin_lo bin_hi Dpad n_own n_streams
//   map           bin_lo bin_hi Dpad n_streams cap_cells
//   tracks_map    bin_lo bin_hi Dpad n_own n_streams cap_cells
//   rows          every solve choice the lookups have a kernel for, one per line, then "end"
#include "../../mcarray_amd/csrc/mvdr_plan.h"

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

std::string dims(const char *name, dim3 d)
{
    char b[64];
    std::snprintf(b, sizeof b, " %s=%u,%u,%u", name, d.x, d.y, d.z);
    return b;
}
std::string launch_text(const MvdrLaunch &l) { return dims("grid", l.grid) + dims("block", l.block) + " lds=" + std::to_string(l.lds) + " attr=" + (l.lds > 64 * 1024 ? "1" : "0"); }
const char *const ANALYSE_FAMILY[] = {"gen", "1024", "512"};
const char *const SOLVE_FAMILY[] = {"hand", "template", "rtf", "rtf_nulls"};
const char *const WEIGHT[] = {"none", "frame", "cell"};
std::string choice_text(const MvdrSolveChoice &k)
{
    char b[160];
    std::snprintf(b, sizeof b, "form=solve_%s Q=%d full=%d S=%d nulls=%d weight=%s noise=%d", SOLVE_FAMILY[(int)k.family], k.Q, (int)k.full, k.S, (int)k.nulls, WEIGHT[(int)k.weight], (int)k.noise);
    return b;
}
void print_scan(const MvdrScanPlan &p, int n_streams)
{
    const int last = n_streams - (n_streams - 1) / p.pass * p.pass;      // streams of the last pass
    std::cout << "chunk0=" << p.b.chunk0 << " n_chunks=" << p.b.n_chunks << " n_slices=" << p.b.n_slices << " nhi=" << p.b.nhi << " nph=" << p.b.nph << " n_tiles=" << p.b.n_tiles
              << " pass=" << p.pass << " lds=" << p.lds << " attr=" << (p.lds > 64 * 1024) << " per_u=" << p.per_u << " per_f=" << p.per_f << " per_part=" << p.per_part
              << dims("tables_grid", p.grid(p.wg_tables, p.pass)) << dims("vectors_grid", p.grid(p.wg_vectors, p.pass)) << dims("scan_grid", p.grid(p.wg_scan, p.pass))
              << dims("last_scan_grid", p.grid(p.wg_scan, last)) << "\n";
}

void print_rows()
{
    for (int fam = 0; fam < 4; ++fam)
        for (int r = 0; r < 4 * 2 * MCA_MAX_SOURCES * 2 * 3 * 2; ++r) {
            const MvdrSolveChoice k{(MvdrSolveFamily)fam, r % 4 + 1, (r / 4 & 1) != 0, r / 8 % MCA_MAX_SOURCES + 1, (r / (8 * MCA_MAX_SOURCES) & 1) != 0,
                                    (MvdrWeight)(r / (16 * MCA_MAX_SOURCES) % 3), r / (48 * MCA_MAX_SOURCES) != 0};
            // (the families without a weight or full argument: one row per kernel, in the form the plan leaves those fields)
            if ((fam >= 2 && k.weight != MvdrWeight::CELL) || !mvdr_solve_choice_row(k)) continue;
            std::cout << choice_text(k) << "\n";
        }
    std::cout << "end\n";
}

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
        MvdrShape s;
        s.N = geti(q, "N"); s.M = geti(q, "M"); s.H = s.N / 2; s.K = s.H + 1; s.tri = s.M * (s.M + 1) / 2; s.max_streams = geti(q, "n_streams");
        while ((1 << s.logH) < s.H) ++s.logH;
        const int n_streams = geti(q, "n_streams"), n_frames = geti(q, "n_frames"), n_sources = geti(q, "n_sources"), n_own = geti(q, "n_own");
        const int lo = geti(q, "bin_lo"), hi = geti(q, "bin_hi"), Dpad = geti(q, "Dpad");
        const size_t cap = (size_t)get(q, "cap_cells");
        if (stage == "rows") print_rows();
        else if (stage == "analyse") {
            const MvdrAnalysePlan p = plan_mvdr_analyse(s, n_streams, n_frames);
            std::cout << "form=analyse_" << ANALYSE_FAMILY[(int)p.family] << " fpb=" << p.fpb << launch_text(p.l) << "\n";
        } else if (stage == "solve_split") {
            const MvdrSolveSplit p = plan_mvdr_solve_split(s, n_streams, geti(q, "n_loop"));
            std::cout << "n_prob=" << p.n_prob << " pieces=" << p.pieces << " main_prob=" << p.main_prob << " tail_prob=" << p.tail_prob << " scratch=" << p.scratch
                      << dims("grid", p.grid) << dims("tail_grid", p.tail_grid) << dims("block", p.block) << "\n";
        } else if (stage == "solve_choice") {
            const MvdrSolveChoice k = plan_mvdr_solve_choice(s, geti(q, "rtf"), n_sources, get(q, "null_gain"), geti(q, "update"), geti(q, "masked"), geti(q, "pf_on"));
            std::cout << choice_text(k) << " have=" << mvdr_solve_choice_row(k) << " lds=" << mvdr_solve_lds(k) << "\n";
        } else if (stage == "rtf") {
            const MvdrRtfPlan p = plan_mvdr_rtf(s, n_streams, n_sources, n_frames, cap);
            std::cout << "fc=" << p.fc << launch_text(p.l) << "\n";
        } else if (stage == "estmask") std::cout << launch_text(plan_mvdr_estmask(s, n_streams, n_frames)).substr(1) << "\n";
        else if (stage == "postfilter") std::cout << launch_text(plan_mvdr_postfilter(s, n_streams, n_sources)).substr(1) << "\n";
        else if (stage == "synth") {
            const MvdrSynthPlan p = plan_mvdr_synth(s, n_streams, n_sources, n_frames);
            std::cout << "ft=" << p.ft << launch_text(p.l) << "\n";
        } else if (stage == "spectrum") print_scan(plan_mvdr_spectrum(s, lo, hi, Dpad, n_streams), n_streams);
        else if (stage == "tracks") print_scan(plan_mvdr_tracks(s, lo, hi, Dpad, n_own, n_streams), n_streams);
        else if (stage == "map") print_scan(plan_mvdr_map(s, lo, hi, Dpad, n_streams, cap), n_streams);
        else if (stage == "tracks_map") print_scan(plan_mvdr_tracks_map(s, lo, hi, Dpad, n_own, n_streams, cap), n_streams);
        else { std::cerr << "unknown stage " << stage << "\n"; return 2; }
    }
    return 0;
}
