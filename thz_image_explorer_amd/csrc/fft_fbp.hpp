// fft_fbp.hpp — "FBP" kernels: chirp-z over the mixed-radix P core, for the trace lengths a tilted real scan lands on.
//
// A scan of 1001 samples whose Tilt Compensation is not zero is re-laid on an axis of 1001 + 2 steps samples
// (tilt_compensation.rs:104-217): 1025 ... 1280 for every tilt up to 4.8 degrees on a 50 mm x 50 mm scan.  Those
// lengths are odd and almost all carry a large prime factor, so none has a direct mixed-radix plan, and the chirp-z
// kernels over the F core (fft_fb.hpp) can only offer them the next power of two, M = 4096, as two 2048-point core
// runs per transform, two waves per pair of traces and two launches per chain.  The convolution needs M >= 2 nt - 1
// only, and the P core (fft_p.hpp: PDft<R>, PPlan, PAddr, p_pass1_round, p_pass23) transforms any product of three
// radices in one LDS buffer per wave, natural order in and out:
//     M = 2304 = 12 x 12 x 16   for 1024 < nt <= 1152
//     M = 2560 = 16 x 16 x 10   for 1152 < nt <= 1280
// One wave per PAIR of traces, the whole chain in ONE launch, as k_fb:
//   forward   z[n] = (x1[n] s1 + i x2[n] s2) pre[n] w[n], n < nt (PairScale: s = 2^-e of the trace's own largest
//             windowed sample) -> pass 1 straight from the loads -> passes 2, 3 -> A[k]
//   multiply  by FFT_M(b) / M where pass 1 of the second transform reads its inputs (pass 1 is in place per
//             butterfly: it reads buf[m + M1 j1] and writes buf[m + M1 k1]), swapped, so that the inverse convolution
//             transform runs through the same forward passes -> passes 2, 3 -> swap(c[k])
//   spectrum  F[k] = swap(c[k]) w[k], k < nt; X1, X2 from F[k], F[nt-k]; fb_finish_bins (256-bin groups, phases
//             before the band pass); the masked spectra go back to the buffer
//   inverse   the same four passes on conj(Y1full + i Y2full) w, its own PairScale taken on the MASKED spectra;
//             y1 = Re U / nt, y2 = -Im U / nt, post window, stores, intensity
// nt <= M / 2: the upper half of the first transform's pass-1 inputs (j1 >= R1 / 2) is zero in both directions, so
// only the lower half is loaded and the radix-R1 butterfly is the half-filled form (FBPHalf).  That is also
// what lets the inverse read all of its packed inputs into registers before pass 1 overwrites the buffer.
//
// LDS per block: [T1: M cx][T2: R2 R3 cx][per wave: M cx][mask nf][pre nt][post nt] — 31.5 KB + 18.0 KB per wave at
// M = 2304 (7 waves in 160 KB), 34.5 KB + 20.0 KB at M = 2560 (6 waves); the block is sized for the longest trace of
// its M.
//
// Three compile-time extras of the fused chain (k_fbp<P, kPipe, TILT, CM, SUMS>; the plain chain and the stage forms
// are the instantiations without them and carry none of their code):
//   TILT  the Tilt Compensation folded into the forward loads (FBPTilt): sample n of pixel p is what k_tilt would have
//         written to the extended cube — src[p][0] in front of the insert index, src[p][n - ins] taper[n - ins] behind
//         it, 0 behind the trace — one f32 multiply in front of the window's, so every output is the staged path's bit
//         for bit.  The taper is read from memory (cache-resident: 4 KB for the whole launch); LDS has no room for it.
//   CM    nf complex multipliers on top of the real mask, as k_p's: [mask nf] becomes [m H: nf cx] (2 320 / 2 576 B
//         more, still 7 / 6 waves), stored spectrum X (m H), amplitude |X m H|, phases of X, real bins' Im +0.
//   SUMS  the launch's sums of the stored amplitudes and unwrapped phases.  A lane owns bins 256 g + 4 lane + c of the
//         three epilogue groups, so a wave keeps 24 accumulators in registers over all of its trips and stores ONE row
//         of A.sum_partial at the end (grid x waves rows of 2 nf floats, every entry written): no LDS, no tickets, no
//         barrier, and the order of every bin's additions is fixed.
#pragma once

#include "fft_fb.hpp"
#include "fft_p.hpp"

namespace thz {

using FBPPlan2304 = PPlan<12, 12, 16>;
using FBPPlan2560 = PPlan<16, 16, 10>;

template <class P>
struct FBPLayout {
    static constexpr int M = P::N;
    static constexpr int kMaxNt = M / 2;  // 2 nt - 1 <= M
    static constexpr int pad4(int v) { return (v + 3) & ~3; }
    static constexpr size_t lds_bytes(int waves, int nt, bool cm = false)
    {
        return (size_t)(P::T1_ENTRIES + P::T2_ENTRIES + waves * P::WAVE_ENTRIES) * sizeof(cx)
               + (size_t)((cm ? 2 : 1) * pad4(nt / 2 + 1) + 2 * pad4(nt)) * sizeof(float);
    }
    // waves of a block: as many as LDS holds next to the tables at the longest trace of this M
    static constexpr int waves()
    {
        int w = 16;
        while (w > 1 && lds_bytes(w, kMaxNt) > (size_t)160 * 1024) --w;
        return w;
    }
    static constexpr int kGroups = 3;  // epilogue groups of 256 bins: 513 <= nf <= 641 for every length of these plans
};

template <int R, int J>
struct FBPTwist {  // W_R^J as compile-time constants
    static constexpr float c = PTrig<R>::c(J), s = PTrig<R>::s(J);
};

// pass 1 of one round when z[n] = 0 from N / 2 on, i.e. v[j1] = 0 for j1 >= R1 / 2: one decimation-in-frequency step
// on the half-filled input,  Y[2 k] = DFT_H(x)[k],  Y[2 k + 1] = DFT_H(x[j] W_R1^j)[k],  H = R1 / 2 — two half-length
// butterflies without the R1 additions in front of them.  Writes as p_pass1_round does.
template <class P>
struct FBPHalf {
    static constexpr int R1 = P::R1, H = R1 / 2, M1 = P::M1;
    static_assert(R1 % 2 == 0, "the half-filled butterfly needs an even first radix");
    template <int... J>
    static __device__ __forceinline__ void twist(const cx (&x)[H], cx (&o)[H], std::integer_sequence<int, J...>)
    {
        ((o[J] = J == 0 ? x[0] : cx_mul(x[J], cx{FBPTwist<R1, J>::c, -FBPTwist<R1, J>::s})), ...);
    }
    static __device__ __forceinline__ void run(cx (&x)[H], cx *buf, const cx *t1, int m, int lb, bool on)
    {
        cx o[H];
        twist(x, o, std::make_integer_sequence<int, H>{});
        PDft<H>::run(x);
        PDft<H>::run(o);
        if (on) {
            buf[lb] = x[0];
#pragma unroll
            for (int k = 0; k < H; ++k) {
                if (k) buf[lb + 2 * k * M1] = cx_mul(x[k], t1[2 * k * M1 + m]);
                buf[lb + (2 * k + 1) * M1] = cx_mul(o[k], t1[(2 * k + 1) * M1 + m]);
            }
        }
    }
};

// The second transform of a convolution: buf holds A[k] in natural order; pass 1 reads A[n] bf[n] swapped, in place
// per butterfly, passes 2 and 3 leave swap(c[k]) in natural order.  Ends with wave_sync() (p_pass23).
template <class P>
__device__ __forceinline__ void fbp_multiply_transform(cx *buf, const cx *__restrict__ bf, const cx *t1, const cx *t2,
                                                       const PAddr<P, 1> &ad, int lane)
{
    constexpr int R1 = P::R1, M1 = P::M1, RD1 = PAddr<P, 1>::RD1;
#pragma unroll
    for (int i = 0; i < RD1; ++i) {
        const bool on = lane + kWave * i < P::B1;
        const unsigned bl = (unsigned)ad.m1[i];
        cx v[R1];
#pragma unroll
        for (int j1 = 0; j1 < R1; ++j1) {
            const cx t = cx_mul(buf[ad.l1[i] + M1 * j1], ld_off(bf, bl + (unsigned)(M1 * j1)));
            v[j1] = cx{t.y, t.x};
        }
        p_pass1_round<P>(v, buf, t1, ad.m1[i], ad.l1[i], on);
        THZ_SCHED_FENCE();
    }
    p_pass23<P, 1>(buf, t2, ad, lane);
}

// A.pre_win2 (forward only): a second window behind pre_win, applied as its own f32 multiply; A.data_out (forward
// only): the windowed traces, the stage's `data` output.
template <class P, int MODE, bool TILT = false, bool CM = false, bool SUMS = false>
__global__ __launch_bounds__(FBPLayout<P>::waves() * kWave) void k_fbp(FBArgs A, PTables T, FBPTilt TL)
{
    static_assert(MODE == kPipe || !(TILT || CM || SUMS), "tilt gather, complex multiplier and sums: the fused chain");
    static_assert(FBPLayout<P>::lds_bytes(FBPLayout<P>::waves(), FBPLayout<P>::kMaxNt, true) <= (size_t)160 * 1024,
                  "the multiplier table fits next to the plain chain's waves");
    THZ_DYN_LDS(lds);
    constexpr int R1 = P::R1, H1 = R1 / 2, M1 = P::M1, WE = P::WAVE_ENTRIES;
    constexpr int RD1 = PAddr<P, 1>::RD1;
    using LY = FBPLayout<P>;
    const int L = A.nt, nf = A.nf;
    const int lane = lane_id();
    const int wib = THZ_UNIFORM((int)(threadIdx.x >> 6));
    const int wpb = (int)(blockDim.x >> 6);
    cx *t1 = reinterpret_cast<cx *>(lds);
    cx *t2 = t1 + P::T1_ENTRIES;
    cx *buf = t2 + P::T2_ENTRIES + (size_t)wib * WE;
    float *mask_s = reinterpret_cast<float *>(t2 + P::T2_ENTRIES + (size_t)wpb * WE);
    float *pre_s = mask_s + (CM ? 2 : 1) * LY::pad4(nf);
    float *post_s = pre_s + LY::pad4(L);  // the forward kernel keeps its second window here
    for (int i = (int)threadIdx.x; i < P::T1_ENTRIES; i += (int)blockDim.x) t1[i] = T.t1[i];
    for (int i = (int)threadIdx.x; i < M1; i += (int)blockDim.x) t2[i] = T.t2[i];
    if constexpr (CM) {
        cx *cm = reinterpret_cast<cx *>(mask_s);
        for (int i = (int)threadIdx.x; i < nf; i += (int)blockDim.x) {
            const float m = A.mask[i];
            const cx h = A.cmask[i];
            cm[i] = cx{h.x * m, h.y * m};
        }
    } else {
        for (int i = (int)threadIdx.x; i < nf; i += (int)blockDim.x) mask_s[i] = A.mask[i];
    }
    for (int i = (int)threadIdx.x; i < L; i += (int)blockDim.x) {
        pre_s[i] = A.pre_win ? A.pre_win[i] : 1.0f;
        if constexpr (MODE == kFwd) post_s[i] = A.pre_win2 ? A.pre_win2[i] : 1.0f;
        else post_s[i] = A.post_win ? A.post_win[i] : 1.0f;
    }
    __syncthreads();

    PAddr<P, 1> ad;
    ad.init(lane);
    const DivConst by_nt((float)L);
    const int n_groups = (nf + 255) / 256;  // epilogue groups of 256 bins: bin = 256 g + 4 lane + c
    const int half = L / 2;
    const float sgn = (L & 1) ? -1.0f : 1.0f;  // w[nt-k] = sgn * w[k]
    const int y2_base = (L + 4) & ~3;          // Y2[k] lives at y2_base + k: behind everything F uses (< 3 nt / 2 + 4 < M)
    const size_t n_pairs = (A.npix + 1) / 2;
    const size_t stride = (size_t)gridDim.x * wpb;
    // SUMS: this wave's sums over all of its trips, [group][bin of the lane's quad]: amplitudes | unwrapped phases
    constexpr int NG = LY::kGroups;
    float sum_a[NG][4], sum_p[NG][4];
    if constexpr (SUMS) {
#pragma unroll
        for (int g = 0; g < NG; ++g)
#pragma unroll
            for (int c = 0; c < 4; ++c) sum_a[g][c] = sum_p[g][c] = 0.0f;
    }

    for (size_t q = (size_t)blockIdx.x * wpb + wib; q < n_pairs; q += stride) {
        const size_t p = 2 * q;
        const bool has2 = p + 1 < A.npix;  // wave-uniform
        ad.refresh();
        const cx *t1l = launder_uniform((const cx *)t1);
        const cx *t2l = launder_uniform((const cx *)t2);
        const cx *wl = launder_uniform(A.w);
        const cx *bf = launder_uniform(A.bf);
        const float *pre_l = launder_uniform((const float *)pre_s);
        const float *post_l = launder_uniform((const float *)post_s);
        const float *mask_l = launder_uniform((const float *)mask_s);
        const int lb4 = launder_v(4 * lane), lb1 = launder_v(lane);
        unsigned ym1 = 0u, ym2 = 0u;  // largest |component| of the two masked spectra (the inverse's PairScale)

        if constexpr (MODE != kInv) {
            // ---- z[n] = (x1[n] + i x2[n]) pre[n] w[n], n = M1 j1 + m, j1 < R1 / 2 (zero from nt on).  Branch-free:
            // indices are clamped and the value selected, every load of the pair is issued before the first use.
            // The windowed samples come first and each trace's largest |value| is taken (PairScale); the chirp multiply
            // follows once both scales are known.
            const size_t row = TILT ? (size_t)TL.nt_in : (size_t)L;
            const float *x1 = (TILT ? TL.src : A.in) + p * row;
            const float *x2 = has2 ? x1 + row : x1;
            float xa[RD1][H1], xb[RD1][H1];
            if constexpr (TILT) {
                // the extended trace as k_tilt lays it out, gathered: index clamped into the source trace, value
                // selected — in front of the insert index the trace's first sample (untapered), behind the trace zero.
                // The two traces of a pair have their own insert indices (wave-uniform).  Every sample load of the pair
                // is issued first, as in the plain chain; the taper (cache-resident) follows round by round
                const int NI = TL.nt_in;
                const int in1 = THZ_UNIFORM(TL.ins[p]), in2 = THZ_UNIFORM(TL.ins[has2 ? p + 1 : p]);
                const float *tp = launder_uniform(TL.taper);
#pragma unroll
                for (int i = 0; i < RD1; ++i)
#pragma unroll
                    for (int j = 0; j < H1; ++j) {
                        const int n = M1 * j + ad.m1[i];
                        const int nn = n < L ? n : L - 1;
                        const int j1 = nn - in1, j2 = nn - in2;
                        xa[i][j] = ld_off(x1, (unsigned)(j1 < 0 ? 0 : (j1 < NI ? j1 : NI - 1)));
                        xb[i][j] = ld_off(x2, (unsigned)(j2 < 0 ? 0 : (j2 < NI ? j2 : NI - 1)));
                    }
#pragma unroll
                for (int i = 0; i < RD1; ++i) {
                    float ta[H1], tb[H1];
#pragma unroll
                    for (int j = 0; j < H1; ++j) {
                        const int n = M1 * j + ad.m1[i];
                        const int nn = n < L ? n : L - 1;
                        const int j1 = nn - in1, j2 = nn - in2;
                        ta[j] = ld_off(tp, (unsigned)(j1 < 0 ? 0 : (j1 < NI ? j1 : NI - 1)));
                        tb[j] = ld_off(tp, (unsigned)(j2 < 0 ? 0 : (j2 < NI ? j2 : NI - 1)));
                    }
#pragma unroll
                    for (int j = 0; j < H1; ++j) {
                        const int n = M1 * j + ad.m1[i];
                        const int nn = n < L ? n : L - 1;
                        const int j1 = nn - in1, j2 = nn - in2;
                        xa[i][j] = j1 < 0 ? xa[i][j] : (j1 < NI ? xa[i][j] * ta[j] : 0.0f);
                        xb[i][j] = j2 < 0 ? xb[i][j] : (j2 < NI ? xb[i][j] * tb[j] : 0.0f);
                    }
                }
            } else {
#pragma unroll
                for (int i = 0; i < RD1; ++i)
#pragma unroll
                    for (int j = 0; j < H1; ++j) {
                        const int n = M1 * j + ad.m1[i];
                        const unsigned nn = (unsigned)(n < L ? n : L - 1);
                        xa[i][j] = ld_off(x1, nn);
                        xb[i][j] = ld_off(x2, nn);
                    }
            }
            unsigned ma = 0u, mb = 0u;
#pragma unroll
            for (int i = 0; i < RD1; ++i) {
#pragma unroll
                for (int j = 0; j < H1; ++j) {
                    const int n = M1 * j + ad.m1[i];
                    const int nn = n < L ? n : L - 1;
                    float a = xa[i][j] * pre_l[nn], b = xb[i][j] * pre_l[nn];
                    if constexpr (MODE == kFwd) {
                        if (A.pre_win2) {  // uniform
                            a *= post_l[nn];
                            b *= post_l[nn];
                        }
                        // the stage's windowed-trace output (uniform pointer); a lane without a butterfly does not store
                        if (A.data_out && lane + kWave * i < P::B1 && n < L) {
                            float *o = A.data_out + p * (size_t)L;
                            o[n] = a;
                            if (has2) o[L + n] = b;
                        }
                    }
                    xa[i][j] = n < L ? a : 0.0f;
                    xb[i][j] = (n < L && has2) ? b : 0.0f;
                    ma = umax(ma, abs_bits(xa[i][j]));
                    mb = umax(mb, abs_bits(xb[i][j]));
                }
            }
            const PairScale e1(wave_reduce_max_u32(ma)), e2(wave_reduce_max_u32(mb));
            const bool any_bad = e1.bad || e2.bad;  // wave-uniform and rare: a non-finite trace enters as zeros
#pragma unroll
            for (int i = 0; i < RD1; ++i) {
                const bool on = lane + kWave * i < P::B1;
                cx wv[H1], v[H1];
#pragma unroll
                for (int j = 0; j < H1; ++j) {
                    const int n = M1 * j + ad.m1[i];
                    wv[j] = ld_off(wl, (unsigned)(n < L ? n : L - 1));
                }
#pragma unroll
                for (int j = 0; j < H1; ++j) {
                    cx z = cx{xa[i][j] * e1.in, xb[i][j] * e2.in};
                    if (any_bad) z = cx{e1.bad ? 0.0f : z.x, e2.bad ? 0.0f : z.y};
                    v[j] = cx_mul(z, wv[j]);
                }
                FBPHalf<P>::run(v, buf, t1l, ad.m1[i], ad.l1[i], on);
                THZ_SCHED_FENCE();
            }
            p_pass23<P, 1>(buf, t2l, ad, lane);
            fbp_multiply_transform<P>(buf, bf, t1l, t2l, ad, lane);  // buf[k] = swap(c[k])

            // ---- spectrum epilogue: F[k] = w[k] c[k]; X1 = (F[k] + conj F[nt-k]) / 2, X2 = (F[k] - conj F[nt-k]) / 2i
            {
                const float h1 = 0.5f * e1.out, h2 = 0.5f * e2.out;
                FBUnwrap u1, u2;
                // SUMS: the groups unrolled, so that the accumulators of a group are registers of their own
                const int g_end = SUMS ? NG : n_groups;
                constexpr int kUnrollGroups = SUMS ? NG : 1;
#pragma unroll kUnrollGroups
                for (int g = 0; g < g_end; ++g) {
                    if constexpr (SUMS)
                        if (g >= n_groups) continue;  // (uniform; never for the lengths of these plans)
                    const int k0 = 256 * g + lb4;
                    cx X1[4], X2[4], h[4];
                    float m[4];
                    bool ok[4], rb[4];
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const int k = k0 + c;
                        ok[c] = k < nf;
                        const int kc = ok[c] ? k : nf - 1;
                        // F[nt] = F[0].  A bin that does not exist reads slot k (< 768 < nt) twice: nobody writes there
                        // during the epilogue, so no lane reads what another lane is writing
                        const int km = ok[c] ? (k == 0 ? 0 : L - k) : k;
                        const cx wk = ld_off(wl, (unsigned)kc);
                        const cx s = buf[k], sm = buf[km];
                        const cx Fk = cx_mul(cx{s.y, s.x}, wk);
                        const cx wm = k == 0 ? wk : cx{sgn * wk.x, sgn * wk.y};
                        const cx Fm = cx_mul(cx{sm.y, sm.x}, wm);
                        // conj(Fm) = (Fm.x, -Fm.y); the 1/2 carries each trace's 2^e (PairScale)
                        X1[c] = cx{h1 * (Fk.x + Fm.x), h1 * (Fk.y - Fm.y)};
                        // (Fk - conj Fm) / 2i = (-i/2) (dx + i dy) = (dy/2, -dx/2)
                        X2[c] = cx{h2 * (Fk.y + Fm.y), -h2 * (Fk.x - Fm.x)};
                        if constexpr (CM) h[c] = reinterpret_cast<const cx *>(mask_l)[kc];
                        else m[c] = mask_l[kc];
                        // real input: DC / Nyquist bins are real, with a POSITIVE zero as imaginary part; a zero trace's
                        // spectrum is +0.0 — both on the bit pattern (p_zero_if)
                        const bool real_bin = k == 0 || ((L & 1) == 0 && k == nf - 1);
                        X1[c] = cx{p_zero_if(X1[c].x, e1.zero), p_zero_if(X1[c].y, real_bin || e1.zero)};
                        X2[c] = cx{p_zero_if(X2[c].x, e2.zero), p_zero_if(X2[c].y, real_bin || e2.zero)};
                        rb[c] = real_bin;
                    }
                    const size_t o1 = p * (size_t)nf + k0;
                    cx Y1[4], Y2[4];  // the multiplied spectra (CM)
                    if constexpr (CM) {
                        fb_finish_bins_c(X1, h, rb, ok, g, lane, u1, A.fft_out ? A.fft_out + o1 : nullptr,
                                         A.amp_out ? A.amp_out + o1 : nullptr, A.ph_out ? A.ph_out + o1 : nullptr, Y1);
                        if (has2)
                            fb_finish_bins_c(X2, h, rb, ok, g, lane, u2, A.fft_out ? A.fft_out + o1 + nf : nullptr,
                                             A.amp_out ? A.amp_out + o1 + nf : nullptr, A.ph_out ? A.ph_out + o1 + nf : nullptr, Y2);
                    } else {
                        fb_finish_bins(X1, m, ok, g, lane, u1, A.fft_out ? A.fft_out + o1 : nullptr,
                                       A.amp_out ? A.amp_out + o1 : nullptr, A.ph_out ? A.ph_out + o1 : nullptr);
                        if (has2)
                            fb_finish_bins(X2, m, ok, g, lane, u2, A.fft_out ? A.fft_out + o1 + nf : nullptr,
                                           A.amp_out ? A.amp_out + o1 + nf : nullptr, A.ph_out ? A.ph_out + o1 + nf : nullptr);
                    }
                    if constexpr (SUMS) {
                        // first trace, then second: u.a / u.y are 0 where the bin does not exist
#pragma unroll
                        for (int c = 0; c < 4; ++c) {
                            sum_a[g][c] += u1.a[c];
                            sum_p[g][c] += u1.y[c];
                        }
                        if (has2) {
#pragma unroll
                            for (int c = 0; c < 4; ++c) {
                                sum_a[g][c] += u2.a[c];
                                sum_p[g][c] += u2.y[c];
                            }
                        }
                    }
                    // masked spectra for the inverse: Y1[k] over c[k] — only its owner reads slot k or nt-k — and
                    // Y2[k] behind everything F uses.  The products are the stored ones (rounded before anything is
                    // added to them: they pass through LDS), so that the inverse transforms exactly the spectrum that
                    // was stored and a later k_fbp<kInv> on it lands on the same samples.
                    if constexpr (MODE == kPipe) {
#pragma unroll
                        for (int c = 0; c < 4; ++c)
                            if (ok[c]) {
                                const cx y1 = CM ? Y1[c] : cx{X1[c].x * m[c], X1[c].y * m[c]};
                                // a missing second trace is exactly zero, as in the stand-alone inverse
                                const cx y2 = !has2 ? cx{0.0f, 0.0f} : CM ? Y2[c] : cx{X2[c].x * m[c], X2[c].y * m[c]};
                                ym1 = umax(ym1, umax(abs_bits(y1.x), abs_bits(y1.y)));
                                ym2 = umax(ym2, umax(abs_bits(y2.x), abs_bits(y2.y)));
                                buf[k0 + c] = y1;
                                buf[y2_base + k0 + c] = y2;
                            }
                    }
                }
            }
            wave_sync();
        } else {
            // inverse only: the two spectra from memory into the slots the fused chain leaves them in;
            // DC (and Nyquist for even nt) imaginary parts are ignored like realfft's C2R does
            const cx *f1 = A.fft_in + p * (size_t)nf;
            for (int k = lb1; k < nf; k += kWave) {
                cx y1 = ld_off(f1, (unsigned)k);
                cx y2 = has2 ? ld_off(f1, (unsigned)(nf + k)) : cx{0.0f, 0.0f};
                if (k == 0 || ((L & 1) == 0 && k == nf - 1)) {
                    y1.y = 0.0f;
                    y2.y = 0.0f;
                }
                ym1 = umax(ym1, umax(abs_bits(y1.x), abs_bits(y1.y)));
                ym2 = umax(ym2, umax(abs_bits(y2.x), abs_bits(y2.y)));
                buf[k] = y1;
                buf[y2_base + k] = y2;
            }
            wave_sync();
        }
        if constexpr (MODE == kFwd) continue;
        // each masked spectrum's PairScale: applied as it is packed, undone on the window post[n]
        const PairScale e1(wave_reduce_max_u32(ym1)), e2(wave_reduce_max_u32(ym2));
        // the butterfly maps made opaque again: otherwise the fused chain keeps every clamped index of the forward
        // loads alive through the whole forward transform for the packing below (and spills)
        ad.refresh();

        // ---- inverse: a'[n] = conj(Y1full[n] + i Y2full[n]) w[n];  Yfull[n] = Y[n] (n <= nt/2), conj(Y[nt-n]) above.
        // Every round's inputs are read before pass 1 writes anything (its outputs land in other rounds' inputs)
        {
            cx v[RD1][H1];
#pragma unroll
            for (int i = 0; i < RD1; ++i) {
                cx wv[H1];
#pragma unroll
                for (int j = 0; j < H1; ++j) {
                    const int n = M1 * j + ad.m1[i];
                    wv[j] = ld_off(wl, (unsigned)(n < L ? n : L - 1));
                }
#pragma unroll
                for (int j = 0; j < H1; ++j) {
                    const int n = M1 * j + ad.m1[i];
                    const int nn = n < L ? n : L - 1;
                    const bool low = nn <= half;
                    const int kk = low ? nn : L - nn;
                    cx y1 = buf[kk], y2 = buf[y2_base + kk];
                    y1 = e1.bad ? cx{0.0f, 0.0f} : cx{y1.x * e1.in, y1.y * e1.in};
                    y2 = e2.bad ? cx{0.0f, 0.0f} : cx{y2.x * e2.in, y2.y * e2.in};
                    // Yfull = low ? Y : conj(Y);  G = Y1full + i Y2full;  conj(G) = conj(Y1full) - i conj(Y2full)
                    // low : conj(Y1) - i conj(Y2) = (y1.x - y2.y, -y1.y - y2.x)
                    // high: Y1 - i Y2             = (y1.x + y2.y,  y1.y - y2.x)
                    const cx gc = low ? cx{y1.x - y2.y, -y1.y - y2.x} : cx{y1.x + y2.y, y1.y - y2.x};
                    const cx t = cx_mul(gc, wv[j]);
                    v[i][j] = n < L ? t : cx{0.0f, 0.0f};
                }
                THZ_SCHED_FENCE();
            }
            wave_sync();
#pragma unroll
            for (int i = 0; i < RD1; ++i) {
                const bool on = lane + kWave * i < P::B1;
                FBPHalf<P>::run(v[i], buf, t1l, ad.m1[i], ad.l1[i], on);
                THZ_SCHED_FENCE();
            }
        }
        p_pass23<P, 1>(buf, t2l, ad, lane);
        fbp_multiply_transform<P>(buf, bf, t1l, t2l, ad, lane);

        // ---- U[n] = w[n] c'[n]:  y1 = Re U / nt, y2 = -Im U / nt, each times post[n]; images = sum y^2
        {
            float *o1 = A.data_out + p * (size_t)L;
            float acc1 = 0.0f, acc2 = 0.0f;
#pragma unroll 4
            for (int n = lb1; n < L; n += kWave) {
                const cx s = buf[n];
                const cx wv = ld_off(wl, (unsigned)n);
                const cx U = cx_mul(cx{s.y, s.x}, wv);
                const float pw = post_l[n];
                const float v1 = by_nt(U.x) * (pw * e1.out);
                o1[n] = v1;
                acc1 += v1 * v1;
                if (has2) {
                    const float v2 = by_nt(-U.y) * (pw * e2.out);
                    o1[L + n] = v2;
                    acc2 += v2 * v2;
                }
            }
            if (A.img) {
                acc1 = wave_reduce_add(acc1);
                acc2 = wave_reduce_add(acc2);
                if (lane == 0) {
                    A.img[p] = acc1;
                    if (has2) A.img[p + 1] = acc2;
                }
            }
        }
        wave_sync();
    }
    if constexpr (SUMS) {
        // one row per wave, every entry written (a wave without a pair writes zeros)
        float *row = A.sum_partial + ((size_t)blockIdx.x * wpb + wib) * (size_t)(2 * nf);
#pragma unroll
        for (int g = 0; g < NG; ++g)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int k = 256 * g + 4 * lane + c;
                if (k < nf) {
                    row[k] = sum_a[g][c];
                    row[nf + k] = sum_p[g][c];
                }
            }
    }
}

}  // namespace thz
