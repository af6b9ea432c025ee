// kernels.h -- declarations of the kernels defined in kernels_*.hip (instantiated there: explicitly, or by the lookup of their family).
#pragma once
#include "mca_internal.h"
#include "stream_plan.h"

namespace mca {

template <int MT, bool ULA, typename OutT> __global__ void k_stft_phat(StftPhatArgs p);
template <int MT, bool ULA, typename OutT> __global__ void k_stft_phat_few(StftPhatArgs p);
__global__ void k_sum_planes(float *C, long long n4, int planes, long long stride);
__global__ void k_scan_partial(ScanPickArgs p);
__global__ void k_scan_carry(ScanPickArgs p);
template <int PL, int MODE> __global__ void k_scan_pick(ScanPickArgs p);   // PL: positions per lane of the peak pick (2 / 6 / 8, by D); MODE 0 plain, 1 adaptive coarse pass
template <int PL, bool PATCH> __global__ void k_scan_repick(ScanPickArgs p);   // PATCH: also patches the steered rows of the frames that missed their predicted bin
__global__ void k_repair_patch(RepairPatchArgs p);
__global__ void k_hist_list(int *list, int *n_list, int *need, int n_units);      // lazy tails (round 5): settle_history
__global__ void k_hist_settle(const float *e_hist, const float *hist_C, float *state, int *n_list, int D, int Dp, float mu, float omu);
__global__ void k_gate(GateArgs p);
__global__ void k_doa_fill(DoaFillArgs p);
template <int CPW, int OCC> __global__ void k_beamform_ola(BeamformArgs p);
template <typename OutT> __global__ void k_stft_phat_gen(StftPhatArgs p);
template <int MT, bool ULA, typename OutT> __global__ void k_stft_phat_512(StftPhatArgs p);
__global__ void k_beamform_512(BeamformArgs p);
template <int R, typename OutT> __global__ void k_stft_phat_sub2(StftPhatArgs p);
__global__ void k_beamform_gen(BeamformArgs p);
__global__ void k_bf_table(float2 *tab, const float *grid, const double *mic_x, int M, int n_pairs, double unit);
template <bool ODD> __global__ void k_beamform_wave(BeamformWaveArgs p);
template <bool POWER> __global__ void k_stft_phat_wave16(StftPhatArgs p);   // 16-microphone ULA, one fp16 plane
template <int MT, bool ULA, typename OutT, bool MERGE = false> __global__ void k_stft_phat_2048(StftPhatArgs p);   // 2048-sample frames, M <= 8 (kernels_2048.hip)
__global__ void k_bf_table_2048(float2 *tab, const float *grid, const double *mic_x, int M, double unit);
__global__ void k_beamform_wave_2048(BeamformWaveArgs p);
template <int NPT, bool ODD> __global__ void k_beamform_wave_ms(BeamformWaveArgs p);   // several sources, forward transforms shared (M <= 8)
template <int MT, bool ULA, typename OutT, bool PL2, bool POWER, bool NOPHAT, bool MERGE, bool CAND = false, bool FUSE = false> __global__ void k_stft_phat_wave(StftPhatArgs p);
__global__ void k_steer_table(float4 *rows, float2 *q, float *nyq, const float *grid, const double *mic_x, int M, double unit);      // 8-microphone ULA contexts (steer.h)
__global__ void k_steer_patch(SteerPatchArgs p);
__global__ void k_steer_synth(SteerSynthArgs p);
// The kernel of a form (stream_plan.h), each lookup beside its family's source, which instantiates exactly the rows of the family's
// predicate; nullptr: not in the build
const void *stft_wave_kernel(const StftForm &f);          // kernels_wave.hip
const void *stft_wave16_kernel(const StftForm &f);
const void *beamform_wave_kernel(const BeamformForm &f);
const void *beamform_wave_ms_kernel(const BeamformForm &f);
const void *stft_block_kernel(const StftForm &f);         // kernels_stream.hip
const void *stft_few_kernel(const StftForm &f);
const void *stft_512_kernel(const StftForm &f);
const void *stft_sub2_kernel(const StftForm &f);
const void *scan_pick_kernel(const PickForm &f);
const void *scan_repick_kernel(const RepickForm &f);
const void *beamform_ola_kernel(const BeamformForm &f);
const void *stft_2048_kernel(const StftForm &f);          // kernels_2048.hip
const void *stft_gen_kernel(const StftForm &f);           // kernels_generic.hip

__global__ void k_srp_gemm_f32(GemmArgs p);
template <bool SPLIT, int BN> __global__ void k_srp_gemm_f16(GemmArgs p);
__global__ void k_srp_gemm_f16_v2(GemmArgs p);      // hi + lo planes, v_mfma_f32_32x32x16_f16
__global__ void k_srp_gemm_f16_v3(GemmArgs p);      // one plane, v_mfma_f32_16x16x32_f16
__global__ void k_srp_gemm_f16_fold(GemmArgs p);    // one plane, planar rows of a folding context: K half y against the even / odd half-width table
template <int BN> __global__ void k_srp_gemm_repair(GemmArgs p);
const void *srp_gemm_f16_kernel(bool split, int bn);      // kernels_gemm.hip
const void *srp_gemm_repair_kernel(int bn);

template <typename T> struct C2;
template <typename T>
__global__ void k_frame_srp(const C2<T> *X, int K, int D, int P, const int2 *pairs, const float *delays,
                            const T *E_in, T *E_out, T mu, T omu, int no_phat);
template <typename T>
__global__ void k_frame_pick(const T *E, int D, int P, int S, const float *grid, T *doa, T *prob, int *bins);
template <typename T>
__global__ void k_frame_beamform(const C2<T> *X, int M, int K, int fs, const double *mic_x, double doa, C2<T> *Y);
template <typename T> __global__ void k_frame_power(const C2<T> *X, int M, int K, T *out);

__global__ void k_gcc2_scan(Gcc2ScanArgs p);
__global__ void k_gcc2_compact(const unsigned char *voiced, int n_frames, int *vidx, int *nv, const int *post0, int *silence,
                               int windows_to_decay, unsigned char *vreset);
__global__ void k_gcc2_fill(Gcc2FillArgs p);
template <typename TC, typename TA>       // setProbability at caller-given angles (kernels_gcc2_prob.hip)
__global__ void k_gcc2_prob(const TC *corr, long long corr_stride, int D, float step, const float *grid, const TA *doas, TA *probs, int n);
template <typename T>
__global__ void k_frame_gcc2(const T *corr, int D, float step, const float *grid, double doa_prev, double doa_mem, double one_minus_doa_mem,
                             double *res);
template <typename TC, int SLOTS>       // the DOA tracker (kernels_gcc2_track.hip); SLOTS: particles per lane
__global__ void k_gcc2_track(Gcc2TrackArgs p);
__global__ void k_mask_stream(MaskArgs p);
__global__ void k_mask_stream_gen(MaskGenArgs p);
__global__ void k_mask_stream_2048(MaskGenArgs p);
__global__ void k_mask_frame(MaskFrameArgs p);
__global__ void k_mb_analyse(MbAnalyseArgs p);
__global__ void k_mb_analyse_1024(MbAnalyseArgs p, int fpb);
__global__ void k_mb_analyse_512(MbAnalyseArgs p, int fpb);
__global__ void k_mb_scan(MbScanArgs p);
__global__ void k_mb_summary(MbSummaryArgs p);
__global__ void k_mvdr_analyse(MvdrAnalyseArgs p);
__global__ void k_mvdr_analyse_1024(MvdrAnalyseArgs p, int fpb);
__global__ void k_mvdr_analyse_512(MvdrAnalyseArgs p, int fpb);
template <int Q, bool FULL> __global__ void k_mvdr_solve(MvdrSolveArgs p);                 // one look direction, no weights (kernels_mvdr.hip)
const void *mvdr_solve_hand_kernel(int Q, bool full);
// every other solve (mvdr_solve.h; mca_internal.h on the parameters and on mvdr_solve_form, which fixes S1, PF and REUSE per row)
template <int Q, bool FULL, int S, int S1, bool PF, bool NULLS, bool REUSE, MvdrWeight WEIGHT, bool NOISE> __global__ void k_mvdr_solve_t(MvdrSolveArgs p);
// the instantiations of one (WEIGHT, NOISE), each group in a translation unit of its own (kernels_mvdr_solve_*.hip)
template <MvdrWeight WEIGHT, bool NOISE> const void *mvdr_solve_kernel_of(int Q, bool full, int S, bool nulls, int *lds_bytes);
// the solve with the right-hand sides from the steering plane of k_mvdr_rtf (mvdr_solve.h; kernels_mvdr_solve_rtf*.hip)
template <int Q, bool FULL, int S, int S1, bool PF, bool NOISE> __global__ void k_mvdr_solve_rtf_t(MvdrSolveArgs p);
template <bool NOISE> const void *mvdr_solve_rtf_kernel_of(int Q, bool full, int S);
// the same with soft nulls at the vectors of the plane (kernels_mvdr_solve_rtf_nulls*.hip)
template <int Q, int S, int S1, bool PF, bool NOISE> __global__ void k_mvdr_solve_rtf_nulls_t(MvdrSolveArgs p);
template <bool NOISE> const void *mvdr_solve_rtf_nulls_kernel_of(int Q, int S, int *lds_bytes);
template <int Q> __global__ void k_mvdr_rtf(MvdrRtfArgs p);                     // target covariances and estimated steering vectors
template <int Q> __global__ void k_mvdr_rtf_steering(MvdrRtfSteerArgs p);
const void *mvdr_rtf_kernel(int Q, bool steering);                              // kernels_mvdr_rtf.hip
template <int Q> __global__ void k_mvdr_estmask(MvdrEstmaskArgs p);             // update and target masks from the call's spectra
const void *mvdr_estmask_kernel(int Q);                                         // kernels_mvdr_estmask.hip
__global__ void k_mvdr_postfilter(MvdrPostfilterArgs p);                                   // decision-directed Wiener gain on the solve's output
__global__ void k_mvdr_synth(MvdrSynthArgs p);
template <int Q> __global__ void k_mvdr_spectrum(MvdrSpectrumArgs p);                      // Capon spatial spectrum of the held covariance
const void *mvdr_spectrum_kernel(int Q);                                         // kernels_mvdr_spectrum.hip
__global__ void k_mvdr_spectrum_pick(MvdrSpectrumPickArgs p);
const void *mvdr_map_scan_kernel(int Q);                                         // the azimuth x elevation Capon map (kernels_mvdr_map.hip)
__global__ void k_mvdr_map_pick(MvdrMapPickArgs p);
__global__ void k_mvdr_elevations(MvdrElevationsArgs p);                                    // the pairs of MvdrGeometry::slot_el (kernels_mvdr_map.hip)
__global__ void k_mvdr_track_tables(MvdrTrackTablesArgs p);                                 // tracks of the look directions (kernels_mvdr_track.hip)
template <int Q> __global__ void k_mvdr_track_spectrum(MvdrTrackSpectrumArgs p);
const void *mvdr_track_spectrum_kernel(int Q);
__global__ void k_mvdr_track_pick(MvdrTrackPickArgs p);
__global__ void k_mvdr_track_fill(MvdrTrackFillArgs p);
__global__ void k_mvdr_track_seed(MvdrTrackSeedArgs p);
__global__ void k_mvdr_trk2_tables(MvdrTrk2TablesArgs p);                                   // tracks in azimuth and elevation (kernels_mvdr_trk2.hip)
const void *mvdr_trk2_vectors_kernel(int Q);
__global__ void k_mvdr_trk2_scan(MvdrTrk2ScanArgs p);
__global__ void k_mvdr_trk2_pick(MvdrTrk2PickArgs p);
__global__ void k_mvdr_trk2_fill(MvdrTrk2FillArgs p);
__global__ void k_mvdr_trk2_seed(MvdrTrk2SeedArgs p);
__global__ void k_tgcc_frames(TgccFrameArgs p);
__global__ void k_tgcc_frame_f64(const double *Lp, const double *Rp, int W, int nd, int rem, double *res, double *index);
__global__ void k_tgcc_gate(TgccGateArgs p);

}  // namespace mca
