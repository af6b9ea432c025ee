// stream_plan_cli.cpp -- TEST-ONLY (tests/test_stream_plan.py): the launch plans of csrc/stream_plan.h on the CPU.  Host code only: built
// with the HIP compiler's host pass (the plan header needs dim3 and the transforms' constants) and run on a machine without a GPU.
//
// stdin: one query per line, "<stage> key=value ...": the keys are the fields of StreamShape and the arguments of the stage's plan function
// (missing keys are zero / the struct's default).  stdout: one line per query, "key=value ...".
//   analysis            f32 planes n_arrays n_frames list_groups list_cap power fl_merged steer cand_on fl_no_phat
//   contraction         planes rows rows_planned rows_planned_chunk
//   repair_contraction  pass_rows repair_ksplit
//   pick                adaptive n_arrays n_chunks
//   repick              patch n_arrays n_chunks        (may_patch: repick_may_patch)
//   beamform            table out_aligned n_arrays n_frames
//   steer               n_arrays np
//   rows                every row the predicates of the kernel lookups have, one per line, then "end"
#include "../../mcarray_amd/csrc/stream_plan.h"

#include <cstdio>
#include <iostream>
#include <map>
#include <sstream>
#include <string>

using namespace mca;

namespace {

typedef std::map<std::string, long long> Query;
long long get(const Query &q, const char *k, long long dflt = 0) { auto it = q.find(k); return it == q.end() ? dflt : it->second; }

// whether the build has the kernel of an analysis form: the family's predicate
bool stft_form_row(const StftForm &f)
{
    switch (f.family) {
    case StftFamily::WAVE: return stft_wave_row(f.mt, f.ula, f.f32, f.pl2, f.power, f.nophat, f.merge, f.cand, f.fuse);
    case StftFamily::WAVE16: case StftFamily::GEN: return true;
    case StftFamily::N512: return stft_512_row(f.mt);
    case StftFamily::N2048: return stft_2048_row(f.mt, f.ula, f.f32, f.merge);
    case StftFamily::SUB2: return stft_sub2_row(f.mt);
    case StftFamily::BLOCK: return stft_block_row(f.mt, f.ula);
    case StftFamily::FEW: return stft_few_row(f.mt, f.ula);
    }
    return false;
}

StreamShape shape_of(const Query &q)
{
    StreamShape s;
    s.M = (int)get(q, "M"); s.P = (int)get(q, "P"); s.G = (int)get(q, "G"); s.D = (int)get(q, "D"); s.Dp = (int)get(q, "Dp"); s.K = (int)get(q, "K");
    s.N = (int)get(q, "N"); s.H = (int)get(q, "H"); s.Kp = (int)get(q, "Kp"); s.S = (int)get(q, "S", 1); s.prec = (int)get(q, "prec");
    s.ula = get(q, "ula"); s.stream_ok = get(q, "stream_ok", 1); s.generic = get(q, "generic"); s.n512 = get(q, "n512"); s.n2048 = get(q, "n2048");
    s.merged = get(q, "merged"); s.n_merged = (int)get(q, "n_merged"); s.Kp_m = (int)get(q, "Kp_m"); s.fold = get(q, "fold");
    s.tab_planes = (int)get(q, "tab_planes", 1); s.n_cu = (int)get(q, "n_cu", 256); s.bf_pairs = (int)get(q, "bf_pairs");
    s.gate = get(q, "gate"); s.no_phat = get(q, "no_phat");
    return s;
}

const char *const STFT_FAMILY[] = {"wave", "wave16", "512", "2048", "sub2", "gen", "block", "few"};
std::string stft_text(const StftForm &f)
{
    char b[160];
    std::snprintf(b, sizeof b, "form=stft_%s mt=%d ula=%d f32=%d pl2=%d power=%d nophat=%d merge=%d cand=%d fuse=%d", STFT_FAMILY[(int)f.family], f.mt, (int)f.ula,
                  (int)f.f32, (int)f.pl2, (int)f.power, (int)f.nophat, (int)f.merge, (int)f.cand, (int)f.fuse);
    return b;
}
std::string dims(const char *name, dim3 d)
{
    char b[64];
    std::snprintf(b, sizeof b, " %s=%u,%u,%u", name, d.x, d.y, d.z);
    return b;
}
const char *const GEMM_FAMILY[] = {"f32", "f16", "v2", "v3", "fold"};
const char *const BF_FAMILY[] = {"wave_2048", "wave_ms", "wave", "512", "gen", "ola"};

void print_rows()
{
    for (int r = 0; r < 512; ++r) {
        StftForm f;
        f.family = StftFamily::WAVE; f.mt = r & 1 ? 8 : 4; f.ula = r & 2; f.f32 = r & 4; f.pl2 = r & 8; f.power = r & 16; f.nophat = r & 32; f.merge = r & 64; f.cand = r & 128; f.fuse = r & 256;
        if (stft_form_row(f)) std::cout << stft_text(f) << "\n";
    }
    // the other analysis families: the fields a family has no template argument for stay as the plan leaves them, one row per kernel
    auto emit = [](StftFamily fam, int mt, bool ula, bool f32, bool power, bool merge) {
        StftForm f;
        f.family = fam; f.mt = mt; f.ula = ula; f.f32 = f32; f.power = power; f.merge = merge;
        if (stft_form_row(f)) std::cout << stft_text(f) << "\n";
    };
    for (int b = 0; b < 2; ++b) { emit(StftFamily::WAVE16, 0, true, false, b, false); emit(StftFamily::GEN, 0, false, b, false, false); }
    for (int mt = 0; mt <= 16; ++mt)
        for (int r = 0; r < 8; ++r) {
            const bool ula = r & 1, f32 = r & 2, merge = r & 4;
            emit(StftFamily::N2048, mt, ula, f32, false, merge);
            if (merge) continue;
            emit(StftFamily::N512, mt, ula, f32, false, false); emit(StftFamily::BLOCK, mt, ula, f32, false, false); emit(StftFamily::FEW, mt, ula, f32, false, false);
            if (!ula) emit(StftFamily::SUB2, mt, false, f32, false, false);
        }
    for (int pl = 0; pl <= 8; ++pl)
        for (int m = 0; m < 2; ++m)
            if (scan_pl_row(pl)) std::cout << "form=pick pl=" << pl << " mode=" << m << "\n" << "form=repick pl=" << pl << " patch=" << m << "\n";
    for (int bn = 0; bn <= 256; bn += 64)
        if (gemm_f16_row(bn)) std::cout << "form=gemm_f16 split=0 bn=" << bn << "\nform=gemm_f16 split=1 bn=" << bn << "\nform=gemm_repair bn=" << bn << "\n";
    for (int npt = 0; npt <= 5; ++npt)
        for (int odd = 0; odd < 2; ++odd)
            if (beamform_ms_row(npt, odd)) std::cout << "form=bf_wave_ms npt=" << npt << " odd=" << odd << "\n";
    for (int cpw = 0; cpw <= 4; ++cpw)
        for (int occ = 0; occ <= 4; ++occ)
            if (beamform_ola_row(cpw, occ)) std::cout << "form=bf_ola cpw=" << cpw << " occ=" << occ << "\n";
    std::cout << "form=bf_wave odd=0\nform=bf_wave odd=1\nend\n";
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
            q[kv.substr(0, eq)] = std::stoll(kv.substr(eq + 1));
        }
        const StreamShape s = shape_of(q);
        const int n_arrays = (int)get(q, "n_arrays"), n_frames = (int)get(q, "n_frames");
        if (stage == "rows") print_rows();
        else if (stage == "analysis") {
            AnalysisFlags fl;
            fl.power = get(q, "power"); fl.merged = get(q, "fl_merged"); fl.steer = get(q, "steer"); fl.cand_on = get(q, "cand_on"); fl.no_phat = get(q, "fl_no_phat");
            const AnalysisPlan p = plan_analysis(s, get(q, "f32"), (int)get(q, "planes", 1), n_arrays, n_frames, (int)get(q, "list_groups"), (int)get(q, "list_cap"), fl);
            std::cout << stft_text(p.form) << " have=" << stft_form_row(p.form) << dims("grid", p.grid) << dims("block", p.block) << " lds=" << p.lds << " fpb=" << p.fpb
                      << " skew=" << p.skew << " steers=" << p.steers << "\n";
        } else if (stage == "contraction") {
            const ContractionPlan p = plan_contraction(s, (int)get(q, "planes", 1), get(q, "rows"), get(q, "rows_planned"), get(q, "rows_planned_chunk"));
            std::cout << "form=gemm_" << GEMM_FAMILY[(int)p.form.family] << " split=" << p.form.split << " bn=" << p.form.bn
                      << " have=" << (p.form.family != GemmFamily::F16 || gemm_f16_row(p.form.bn)) << dims("grid", p.grid) << dims("block", p.block) << " lds=" << p.lds
                      << " ksplit=" << p.ksplit << "\n";
        } else if (stage == "repair_contraction") {
            const RepairContractionPlan p = plan_repair_contraction(s, get(q, "pass_rows"), (int)get(q, "repair_ksplit"));
            std::cout << "form=gemm_repair bn=" << p.bn << " have=" << gemm_f16_row(p.bn) << " col_tiles=" << p.col_tiles << dims("grid", p.grid) << dims("block", p.block)
                      << dims("patch_grid", p.patch_grid) << dims("patch_block", p.patch_block) << "\n";
        } else if (stage == "pick") {
            const PickPlan p = plan_pick(s, get(q, "adaptive"), n_arrays, (int)get(q, "n_chunks"));
            std::cout << "form=pick pl=" << p.form.pl << " mode=" << p.form.mode << " have=" << scan_pl_row(p.form.pl) << dims("grid", p.grid) << dims("block", p.block)
                      << " lds=" << p.lds << "\n";
        } else if (stage == "repick") {
            const RepickPlan p = plan_repick(s, get(q, "patch"), n_arrays, (int)get(q, "n_chunks"));
            std::cout << "form=repick pl=" << p.form.pl << " patch=" << p.form.patch << " have=" << scan_pl_row(p.form.pl) << dims("grid", p.grid) << dims("block", p.block)
                      << " lds=" << p.lds << " may_patch=" << repick_may_patch(s) << "\n";
        } else if (stage == "beamform") {
            const BeamformPlan p = plan_beamform(s, get(q, "table"), get(q, "out_aligned", 1), n_arrays, n_frames);
            const BeamformFamily fam = p.form.family;
            std::cout << "form=bf_" << BF_FAMILY[(int)fam];
            bool have = true;
            if (fam == BeamformFamily::WAVE_MS) { std::cout << " npt=" << p.form.npt << " odd=" << p.form.odd; have = beamform_ms_row(p.form.npt, p.form.odd); }
            if (fam == BeamformFamily::WAVE) std::cout << " odd=" << p.form.odd;
            if (fam == BeamformFamily::OLA) { std::cout << " cpw=" << p.form.cpw << " occ=" << p.form.occ; have = beamform_ola_row(p.form.cpw, p.form.occ); }
            std::cout << " have=" << have << dims("grid", p.grid) << dims("block", p.block) << " lds=" << p.lds << " ft=" << p.ft << " skew=" << p.skew << " nb=" << p.nb
                      << " s_pass=" << p.s_pass << " unsupported=" << (p.unsupported ? 1 : 0) << " why=" << (p.unsupported ? p.unsupported : "-") << "\n";
        } else if (stage == "steer") {
            const SteerPlan p = plan_steer(s, n_arrays, (int)get(q, "np"));
            std::cout << "ft=" << p.ft << dims("patch_grid", p.patch_grid) << dims("synth_grid", p.synth_grid) << dims("block", p.block) << " lds=" << p.lds << "\n";
        } else { std::cerr << "unknown stage " << stage << "\n"; return 2; }
    }
    return 0;
}
