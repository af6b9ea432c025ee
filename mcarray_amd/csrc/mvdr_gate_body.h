// mvdr_gate_body.h -- the statements of k_mvdr_gated_t and k_mvdr_masked_t, included by mvdr_gate.h into the braces of either behind
// a "constexpr bool MASKED" (text, not a function: the per-frame kernels compile to the instruction streams they had before the
// masked ones existed only as a kernel's own statements -- inlined from a shared function they came out reordered).  The template
// parameters Q, FULL, S, S1, PF, NULLS, REUSE, NOISE and the argument ka are those of the kernel; mvdr_gate.h says what they mean.
    static_assert(!(MASKED && REUSE), "a wave of quads with weights of their own would run both column bodies");
    const MvdrGateArgs &pa = mvdr_gate_args(ka);
    const MvdrSolveArgs &p = pa.s;
    static_assert(S >= 1 && S <= MCA_MAX_SOURCES && S1 >= 1 && S % S1 == 0, "look directions per frame, in whole passes");
    static_assert(!NULLS || (S >= 2 && !FULL), "the nulls need another direction; their kernel has no branch-free M = 4Q form");
    static_assert(NULLS || PF || NOISE || MASKED, "only the nulls kernel, and a NOISE or MASKED row that needs the registers, give up the load a frame ahead");
    constexpr int NE = 2 * Q * (Q + 1);          // row slot q holds 4 (q + 1) entries, starting at 2 q (q + 1)
    constexpr int NP = NULLS ? S * (S - 1) / 2 : 1;   // pairs of look directions
    constexpr bool PASSES = S1 < S;
    // dynamic LDS of the nulls, sized by the launch (mvdr_nulls_lds_bytes)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float2 *Us = reinterpret_cast<float2 *>(smem_raw);      // [q][s][thread]: u_{4q+l}[s] of the thread's problem, by the row's owner
    float2 *Ns = Us + Q * S * 256;                          // [s][thread]: num of every pass (PASSES only)
    float *Ds = reinterpret_cast<float *>(Ns + S * 256);    // [s][thread]: den
    const int tid = threadIdx.x, l = tid & 3;
    const int M = p.M, K = p.K, F = p.n_frames;
    const int piece = (int)(blockIdx.x % (unsigned)p.pieces);
    const int t_first = (int)((long long)piece * F / p.pieces), t_last = (int)((long long)(piece + 1) * F / p.pieces);   // frames this workgroup solves
    const long long total = p.pid0 + p.n_prob;
    const long long pid = p.pid0 + (long long)(blockIdx.x / (unsigned)p.pieces) * 64 + (tid >> 2);
    const bool pv = pid < total;
    const long long pc = pv ? pid : total - 1;   // surplus quads shadow the last problem and store nothing
    const int a = (int)(pc / K), k = (int)(pc - (long long)a * K);

    const int tri = M * (M + 1) / 2;
    float2 *st = p.phi + pc * tri;
    float2 P[NE], L[NE];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int i = 4 * q + l;
#pragma unroll
        for (int m = 0; m < 4 * (q + 1); ++m)
            P[2 * q * (q + 1) + m] = (i < M && m <= i) ? st[i * (i + 1) / 2 + m] : make_float2(0.f, 0.f);
    }
    float tr = p.trace[pc];
    const int nhi = ((K - 1) >> 5) + 1, nph = nhi + 32;
    const float2 *T = p.T + (long long)a * F * S * M * nph + (k >> 5);     // + ((t S + s) M + m) nph: hi factor; + lo_off: lo
    const int lo_off = nhi - (k >> 5) + (k & 31);
    const long long fstride = (long long)K * M;
    const float2 *X = p.X + (long long)a * F * fstride + (long long)k * M + l;
    const float al = p.alpha, oma = p.one_minus_alpha;
    // each kernel forms its own address only: !MASKED update[a F + t], MASKED update[(a F + t) K + k]
    const int uw0 = MASKED ? 0 : a * F;                                     // + t: the weight of the frame, the same for the four lanes (< 2^31: T is larger)
    const float *um = MASKED ? pa.update + ((long long)a * F * K + k) : nullptr;   // + t K: the weight of the cell (64-bit index), the same for the four lanes
    float2 *yo = p.Y + (long long)a * S * F * K + k;                        // + (s F + t) K
    float *pno = mvdr_noise_plane(ka);                                     // NOISE: the same index
    if constexpr (NOISE) pno += (long long)a * S * F * K + k;

    float hp[Q];                                  // REUSE: inverse pivots of the rows of this lane, of the last frame that factorised
    bool have_l = false;                          // REUSE: L and hp are those of PhiL as it stands
#pragma unroll
    for (int q = 0; q < Q; ++q) hp[q] = 0.f;
    float2 xn[Q];                                 // the next frame's spectra, loaded a frame ahead (PF)
#pragma unroll
    for (int q = 0; q < Q; ++q) xn[q] = (PF && (FULL || 4 * q + l < M)) ? X[4 * q] : make_float2(0.f, 0.f);
    for (int t = 0; t < t_last; ++t) {
        float2 x[Q], rd[S1][Q], rx[Q];
        float dsum[Q];
        // the loads of the frame first, the weight among them
        const long long tn = (long long)min(t + 1, t_last - 1) * fstride;
        float w = MASKED ? um[(long long)t * K] : pa.update[uw0 + t];
#pragma unroll
        for (int q = 0; q < Q; ++q) x[q] = PF ? xn[q] : ((FULL || 4 * q + l < M) ? X[(long long)t * fstride + 4 * q] : make_float2(0.f, 0.f));
        if (t >= t_first) {
#pragma unroll
            for (int s = 0; s < S1; ++s) mvdr_steer_rows<Q, FULL>(rd[s], T, (long long)t * S + s, M, nph, lo_off, l);
        }
        if constexpr (PF) {
#pragma unroll
            for (int q = 0; q < Q; ++q) xn[q] = (FULL || 4 * q + l < M) ? X[tn + 4 * q] : make_float2(0.f, 0.f);
        }
        w = fminf(fmaxf(w, 0.f), 1.f);            // NaN -> 0
        const bool frozen = !(w > 0.f);
        if (!frozen) {
            // Phi <- a Phi + b x x^H (the rows of this lane), tr <- a tr + b |x|^2; b = (1 - alpha) u, a = 1 - b, and at u == 1 the
            // context's own 1 - alpha and alpha
            const float bt = w == 1.f ? oma : oma * w, at = w == 1.f ? al : 1.f - oma * w;
            float e = 0.f;
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                const float2 xs = make_float2(bt * x[q].x, bt * x[q].y);
#pragma unroll
                for (int m = 0; m < 4 * (q + 1); ++m)
                    if (FULL || m < M) {
                        const float2 xm = quad_bcast(x[m >> 2], m & 3);
                        float2 &e_ = P[2 * q * (q + 1) + m];
                        e_ = cmacc(make_float2(at * e_.x, at * e_.y), xs, xm);
                        if (q == Q - 1) e = fmaf(xm.x, xm.x, fmaf(xm.y, xm.y, e));
                    }
            }
            tr = fmaf(at, tr, bt * e);
        }
        if (t < t_first) continue;               // (an earlier piece solves this frame)
        const bool reuse = REUSE && frozen && have_l;
        have_l = true;
        // the loading as the unweighted kernels apply it (k_mvdr_solve_sources on why it is spelled out): contracted into the pivot
        // with all columns in one basic block (FULL), rounded on its own behind the "j < M" branches -- read off their disassembly
        float delta = p.loading_over_m * tr;
        asm volatile("" : "+v"(delta));
        const bool silent = !(tr > 1e-30f);       // the same in the four lanes of a quad
        if constexpr (NULLS) {
            // x does not ride the column loop: a further pass and the silence branch read the frame again (k_mvdr_nulls)
#pragma unroll
            for (int q = 0; q < Q; ++q) rx[q] = x[q];
        }

        float2 bq[S];                             // NULLS: b_s = num and G_ss = den of every direction
        float gd[S];
        // one pass per S1 look directions, s0 ... s0 + S1 - 1
#pragma unroll 1
        for (int s0 = 0;;) {
            float2 num[S1];
            float den[S1];
#pragma unroll
            for (int s = 0; s < S1; ++s) { num[s] = make_float2(0.f, 0.f); den[s] = 0.f; }
#pragma unroll
            for (int q = 0; q < Q; ++q) { if (!NULLS) rx[q] = x[q]; dsum[q] = 0.f; }
            float2 *up = Us + s0 * 256 + tid;
            // the columns; SUB: substitutions only, against the held L and inverse pivots
            auto columns = [&](auto subc) __attribute__((always_inline)) {
                constexpr bool SUB = decltype(subc)::value;
                mvdr_static_for<0, 4 * Q>([&](auto jc) __attribute__((always_inline)) {
                    constexpr int j = decltype(jc)::value, jq = j >> 2, jl = j & 3, jo = 2 * jq * (jq + 1);
                    if (FULL || j < M) {
                        // pivot and the substitution values of row j, from its owner
                        float inv;
                        if constexpr (SUB) inv = quad_bcast1<jl>(hp[jq]);
                        else {
                            // (k_mvdr_nulls, left to the compiler: contracted in column 0, and in every column of its two-pass instantiation, rounded on its own elsewhere)
                            const float pjj = (FULL || (NULLS && (PASSES || j == 0))) ? fmaf(p.loading_over_m, tr, P[jo + j].x) : P[jo + j].x + delta;
                            inv = __builtin_amdgcn_rsqf(quad_bcast1<jl>(pjj - dsum[jq]));
                            if constexpr (REUSE) hp[jq] = l == jl ? inv : hp[jq];
                        }
                        float2 uj[S1], vj = quad_bcast(rx[jq], jl);
                        vj = make_float2(vj.x * inv, vj.y * inv);
#pragma unroll
                        for (int s = 0; s < S1; ++s) {
                            uj[s] = quad_bcast(rd[s][jq], jl);
                            uj[s] = make_float2(uj[s].x * inv, uj[s].y * inv);
                            num[s] = cmacc(num[s], vj, uj[s]);                  // conj(u_j) v_j
                            den[s] = fmaf(uj[s].x, uj[s].x, fmaf(uj[s].y, uj[s].y, den[s]));
                        }
                        if constexpr (NULLS) {
                            if (l == jl) {                                      // the row's owner parks u_j for the cross terms
#pragma unroll
                                for (int s = 0; s < S1; ++s) up[(jq * S + s) * 256] = uj[s];
                            }
                        }
                        if constexpr (!SUB) {
                            // L_ij = (Phi_ij - sum_{m<j} L_im conj(L_jm)) / L_jj for the rows below j (rows <= j compute dead values)
                            float2 s_[Q];
#pragma unroll
                            for (int q = jq; q < Q; ++q) s_[q] = P[2 * q * (q + 1) + j];
#pragma unroll
                            for (int m = 0; m < j; ++m) {
                                const float2 r = quad_bcast(L[jo + m], jl);
#pragma unroll
                                for (int q = jq; q < Q; ++q) s_[q] = cnmacc(s_[q], L[2 * q * (q + 1) + m], r);
                            }
#pragma unroll
                            for (int q = jq; q < Q; ++q) {
                                const float2 lq = make_float2(s_[q].x * inv, s_[q].y * inv);
                                L[2 * q * (q + 1) + j] = lq;
                                dsum[q] = fmaf(lq.x, lq.x, fmaf(lq.y, lq.y, dsum[q]));
                            }
                        }
#pragma unroll
                        for (int q = jq; q < Q; ++q) {
                            const float2 lq = L[2 * q * (q + 1) + j];
#pragma unroll
                            for (int s = 0; s < S1; ++s) rd[s][q] = cnmac(rd[s][q], lq, uj[s]);
                            rx[q] = cnmac(rx[q], lq, vj);
                        }
                    }
                });
            };
            if constexpr (REUSE) {
                if (reuse) columns(std::true_type{});
                else columns(std::false_type{});
            } else columns(std::false_type{});
            float2 y[S1];
            float pr = 0.f;                       // NOISE: 1 / den of the direction this lane stores
            if constexpr (!NULLS) {
#pragma unroll
                for (int s = 0; s < S1; ++s) {
                    const float rden = __builtin_amdgcn_rcpf(den[s]);
                    y[s] = make_float2(num[s].x * rden, num[s].y * rden);
                    if constexpr (NOISE) pr = (s == 0 || l == s) ? rden : pr;
                }
            }
            if (NULLS ? silent : !(tr > 1e-30f)) {
                // digital silence so far: w = d/M, the reference's delay-and-sum (Beamformer.cpp:51-71), per direction
                float2 xr[Q];
#pragma unroll
                for (int q = 0; q < Q; ++q) xr[q] = !NULLS ? x[q] : ((FULL || 4 * q + l < M) ? X[(long long)t * fstride + 4 * q] : make_float2(0.f, 0.f));
#pragma unroll
                for (int s = 0; s < S1; ++s) {
                    float2 d[Q];
                    mvdr_steer_rows<Q, FULL>(d, T, (long long)t * S + s0 + s, M, nph, lo_off, l);
                    float2 acc = make_float2(0.f, 0.f);
#pragma unroll
                    for (int q = 0; q < Q; ++q) acc = cmacc(acc, xr[q], d[q]);   // conj(d_i) x_i
                    acc.x += __shfl_xor(acc.x, 1, 4); acc.y += __shfl_xor(acc.y, 1, 4);
                    acc.x += __shfl_xor(acc.x, 2, 4); acc.y += __shfl_xor(acc.y, 2, 4);
                    y[s] = make_float2(acc.x / (float)M, acc.y / (float)M);
                }
                if constexpr (NOISE) pr = 0.f;
            }
            if (!NULLS || silent) {
                // every lane of the quad holds the S1 results: lane s stores direction s0 + s
                float2 ys = y[0];
#pragma unroll
                for (int s = 1; s < S1; ++s) if (l == s) ys = y[s];
                if (l < S1 && pv) {
                    yo[((long long)(s0 + l) * F + t) * K] = ys;
                    if constexpr (NOISE) pno[((long long)(s0 + l) * F + t) * K] = pr;
                }
            }
            if constexpr (NULLS) {
                if constexpr (PASSES) {
#pragma unroll
                    for (int s = 0; s < S1; ++s) { Ns[(s0 + s) * 256 + tid] = num[s]; Ds[(s0 + s) * 256 + tid] = den[s]; }
                } else {
#pragma unroll
                    for (int s = 0; s < S1; ++s) { bq[s] = num[s]; gd[s] = den[s]; }
                }
            }
            s0 += S1;
            if (S1 == S || s0 >= S) break;
            if constexpr (NULLS) {
#pragma unroll
                for (int q = 0; q < Q; ++q) rx[q] = (FULL || 4 * q + l < M) ? X[(long long)t * fstride + 4 * q] : make_float2(0.f, 0.f);
            }
#pragma unroll
            for (int s = 0; s < S1; ++s) mvdr_steer_rows<Q, FULL>(rd[s], T, (long long)t * S + s0 + s, M, nph, lo_off, l);
        }
        if constexpr (NULLS) {
            if (silent) continue;
            if constexpr (PASSES) {
#pragma unroll
                for (int s = 0; s < S; ++s) { bq[s] = Ns[s * 256 + tid]; gd[s] = Ds[s * 256 + tid]; }
            }
            // G_ab = sum_j conj(u_j[a]) u_j[b], a < b: the rows of this lane, then the quad
            float2 c[NP];
#pragma unroll
            for (int i = 0; i < NP; ++i) c[i] = make_float2(0.f, 0.f);
#pragma unroll
            for (int q = 0; q < Q; ++q)
                if (4 * q + l < M) {
                    float2 u[S];
#pragma unroll
                    for (int s = 0; s < S; ++s) u[s] = Us[(q * S + s) * 256 + tid];
#pragma unroll
                    for (int sa = 0; sa < S; ++sa)
#pragma unroll
                        for (int sb = sa + 1; sb < S; ++sb) c[mvdr_pair(S, sa, sb)] = cmacc(c[mvdr_pair(S, sa, sb)], u[sb], u[sa]);
                }
            float rs[S];
            float2 beta[S];
#pragma unroll
            for (int s = 0; s < S; ++s) {
                rs[s] = __builtin_amdgcn_rsqf(gd[s]);
                beta[s] = make_float2(bq[s].x * rs[s], bq[s].y * rs[s]);
            }
#pragma unroll
            for (int sa = 0; sa < S; ++sa)
#pragma unroll
                for (int sb = sa + 1; sb < S; ++sb) {
                    float2 &e_ = c[mvdr_pair(S, sa, sb)];
                    const float ww = rs[sa] * rs[sb];
                    e_ = make_float2(quad_sum(e_.x) * ww, quad_sum(e_.y) * ww);
                }
            const float g = pa.null_gain;
            float2 ys = make_float2(0.f, 0.f);
            mvdr_static_for<0, S>([&](auto sc) __attribute__((always_inline)) {
                constexpr int s = decltype(sc)::value;
                const float2 y = mvdr_null_output<S, s>(c, beta, rs, g);
                if (l == s) ys = y;
            });
            // every lane of the quad holds the S results: lane s stores direction s
            if (l < S && pv) {
                yo[((long long)l * F + t) * K] = ys;
                if constexpr (NOISE) {
                    float gs = gd[0];
#pragma unroll
                    for (int s = 1; s < S; ++s) gs = l == s ? gd[s] : gs;
                    pno[((long long)l * F + t) * K] = __builtin_amdgcn_rcpf(gs);
                }
            }
        }
    }
    if (pv && t_last == F) {
        float2 *so = p.phi_out + (pc - p.out_base) * tri;
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const int i = 4 * q + l;
#pragma unroll
            for (int m = 0; m < 4 * (q + 1); ++m)
                if (i < M && m <= i) so[i * (i + 1) / 2 + m] = P[2 * q * (q + 1) + m];
        }
        if (l == 0) p.trace_out[pc - p.out_base] = tr;
    }
