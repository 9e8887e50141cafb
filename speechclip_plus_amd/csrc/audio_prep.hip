// Raw-audio input of the speech encoder: what the reference's librosa.load(path, sr=16_000) does to a decoded file (avssl/data/base_dataset.py:81,
// example.py:21) - to float, to mono, resample to 16 kHz - on the device, for a ragged batch of PCM utterances of one source rate.  The filter
// is the project's own, in closed form (include/speechclip_hip.h, "Raw-audio input"): a Hann-windowed sinc, six zero crossings, roll-off 0.99,
// as a polyphase table [Q][taps] built in float64 on the host (speechclip_plus_amd/audio_prep.py).  One launch; the kernel also writes the
// zeros behind every utterance, so the caller allocates `out` and nothing else.
//
// Block (tile of outputs, utterance); the host picks the tile per rate so that the window fits.  The table goes to LDS (row stride odd: neighbouring lanes read neighbouring phases),
// then the tile's input window [first tap of the first output, last tap of the last output] - converted to fp32 and down-mixed, zero where
// the index falls outside the utterance: that is the only read of the source, and no sample outside [0, n_in) is loaded.  Each output is one
// fmaf chain over its phase's taps in ascending order, over values that do not depend on the tile or the batch: same input, same bits.
#include "sc_common.h"

namespace {

constexpr int AP_THREADS = 256;

struct ap_desc {                        // one utterance: 5 x int64 (audio_prep.py)
    int64_t src_off, n_in, ch, n_out, row;
};

// frame j of the utterance as mono fp32: int16 -> x / 32768 (exact), channels summed in order, divided by the count
template <bool I16>
__device__ __forceinline__ float ap_mono(const uint8_t* __restrict__ base, int64_t j, int ch) {
    float s;
    if (I16) {
        const int16_t* p = (const int16_t*)base + j * ch;
        s = (float)p[0] * (1.0f / 32768.0f);
        for (int c = 1; c < ch; ++c) s += (float)p[c] * (1.0f / 32768.0f);
    } else {
        const float* p = (const float*)base + j * ch;
        s = p[0];
        for (int c = 1; c < ch; ++c) s += p[c];
    }
    return ch > 1 ? s / (float)ch : s;
}

template <bool I16>
__global__ __launch_bounds__(AP_THREADS) void audio_resample_kernel(const uint8_t* __restrict__ src, int64_t src_bytes, const int64_t* __restrict__ desc,
                                                                    const float* __restrict__ table, const int32_t* __restrict__ first, int P, int Q,
                                                                    int taps, int tile, int win_cap, float* __restrict__ out, int64_t ld_out,
                                                                    int out_rows, int Lout) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const ap_desc d = *(const ap_desc*)(desc + 5 * blockIdx.y);
    const int64_t m0 = (int64_t)blockIdx.x * tile;
    if (d.row < 0 || d.row >= out_rows || m0 >= Lout) return;
    float* orow = out + d.row * ld_out;
    const int64_t m_end = min(m0 + tile, (int64_t)Lout);
    const int esz = I16 ? 2 : 4;
    // an utterance the buffer does not hold (a corrupt descriptor) reads nothing: its row is zeros
    const bool ok = d.ch >= 1 && d.ch <= 8 && d.n_in >= 1 && d.src_off >= 0 && d.src_off % esz == 0 && d.n_in <= (src_bytes - d.src_off) / (d.ch * esz);
    const int64_t n_out = ok ? min(max(d.n_out, (int64_t)0), (int64_t)Lout) : 0;
    const int64_t m_live = min(m_end, n_out);                          // outputs m0 .. m_live - 1 are computed, m_live .. m_end - 1 are zeros
    const int ch = (int)d.ch;
    const uint8_t* base = src + d.src_off;
    if (m_live > m0) {
        if (P == 1 && Q == 1) {                                        // 16 kHz: convert and down-mix, no filter
            for (int64_t m = m0 + threadIdx.x; m < m_live; m += AP_THREADS) orow[m] = m < d.n_in ? ap_mono<I16>(base, m, ch) : 0.f;
        } else {
            const int ts = taps | 1;                                   // LDS row stride of the table
            float* tab = lds;
            float* win = lds + (size_t)Q * ts;
            for (int i = threadIdx.x; i < Q * taps; i += AP_THREADS) {
                const int ph = i / taps;
                tab[ph * ts + (i - ph * taps)] = table[i];
            }
            // start(m) = (m div Q) P + first[m mod Q] does not decrease with m: the window runs from start(m0) to start(m_live - 1) + taps
            // m div Q, m mod Q and (m div Q) P in 64 bits once per block; inside the tile the differences fit 32 bits
            const int64_t q0 = m0 / Q, q1 = (m_live - 1) / Q;
            const int r0 = (int)(m0 - q0 * Q);
            const int f0 = first[r0];
            const int64_t in_lo = q0 * P + f0;
            const int64_t in_hi = q1 * P + first[(int)(m_live - 1 - q1 * Q)] + taps;
            const int wlen = (int)min(max(in_hi - in_lo, (int64_t)0), (int64_t)win_cap);
            for (int w = threadIdx.x; w < wlen; w += AP_THREADS) {
                const int64_t j = in_lo + w;
                win[w] = (j >= 0 && j < d.n_in) ? ap_mono<I16>(base, j, ch) : 0.f;
            }
            __syncthreads();
            const int n_live = (int)(m_live - m0);
            for (int dm = threadIdx.x; dm < n_live; dm += AP_THREADS) {
                const int dq = (r0 + dm) / Q;
                const int ph = r0 + dm - dq * Q;
                const int rel = dq * P + first[ph] - f0;
                float acc = 0.f;
                if (rel >= 0 && rel + taps <= wlen) {
                    const float* h = tab + ph * ts;
                    const float* x = win + rel;
                    for (int t = 0; t < taps; ++t) acc = fmaf(h[t], x[t], acc);
                }
                orow[m0 + dm] = acc;
            }
        }
    }
    for (int64_t m = max(m0, m_live) + threadIdx.x; m < m_end; m += AP_THREADS) orow[m] = 0.f;
}

sc_lds_attr_once ap_lds_i16, ap_lds_f32;

}  // namespace

extern "C" int sc_audio_resample(const void* src, int64_t src_bytes, int32_t is_i16, const int64_t* desc, int32_t n_utt, const float* table,
                                 const int32_t* first, int32_t P, int32_t Q, int32_t taps, int32_t tile, float* out, int64_t ld_out,
                                 int32_t out_rows, int32_t Lout, void* stream) {
    SC_CHECK(src && desc && out, "sc_audio_resample: null pointer");
    SC_CHECK(n_utt > 0 && n_utt < 65536 && src_bytes > 0, "sc_audio_resample: n_utt=%d (1 .. 65535) src_bytes=%lld", n_utt, (long long)src_bytes);
    SC_CHECK(out_rows > 0 && Lout > 0 && ld_out >= Lout, "sc_audio_resample: out_rows=%d Lout=%d ld_out=%lld (rows, Lout >= 1, ld_out >= Lout)",
             out_rows, Lout, (long long)ld_out);
    SC_CHECK(P >= 1 && Q >= 1 && P <= 4096 && Q <= 4096, "sc_audio_resample: P=%d Q=%d (1 .. 4096 each)", P, Q);
    SC_CHECK(tile >= AP_THREADS && tile % AP_THREADS == 0 && tile <= 4096, "sc_audio_resample: tile=%d must be a multiple of %d, at most 4096", tile,
             AP_THREADS);
    SC_CHECK(((uintptr_t)desc % 8) == 0 && ((uintptr_t)out % 4) == 0 && ((uintptr_t)src % 4) == 0,
             "sc_audio_resample: desc must be 8-byte, src and out 4-byte aligned");
    const bool pass = P == 1 && Q == 1;
    int win_cap = 0;
    size_t lds_bytes = 0;
    if (!pass) {
        SC_CHECK(table && first, "sc_audio_resample: a rate other than 16 kHz needs the table and the first-tap offsets");
        SC_CHECK(taps >= 1 && (int64_t)Q * taps * 4 <= 65536, "sc_audio_resample: taps=%d Q=%d: the table [Q][taps] fp32 must be 1 .. 65536 bytes", taps, Q);
        SC_CHECK(((uintptr_t)table % 4) == 0 && ((uintptr_t)first % 4) == 0, "sc_audio_resample: table / first must be 4-byte aligned");
        // the window of a tile: start(m0 + tile - 1) - start(m0) + taps <= ceil((tile - 1) P / Q) + 1 + taps (first[] follows i P / Q to within one sample)
        win_cap = (int)(((int64_t)(tile - 1) * P + Q - 1) / Q) + taps + 2;
        lds_bytes = ((size_t)Q * (taps | 1) + win_cap) * sizeof(float);
        SC_CHECK(lds_bytes <= 160 * 1024 - 1024, "sc_audio_resample: tile=%d at P=%d Q=%d taps=%d needs %zu bytes of LDS", tile, P, Q, taps, lds_bytes);
        if (lds_bytes > 48 * 1024) {
            const hipError_t e = is_i16 ? sc_set_max_lds_once(ap_lds_i16, audio_resample_kernel<true>, 160 * 1024 - 1024)
                                        : sc_set_max_lds_once(ap_lds_f32, audio_resample_kernel<false>, 160 * 1024 - 1024);
            SC_CHECK(e == hipSuccess, "sc_audio_resample: raising the LDS limit failed: %s", hipGetErrorString(e));
        }
    }
    const dim3 grid((Lout + tile - 1) / tile, n_utt);
    if (is_i16)
        hipLaunchKernelGGL(audio_resample_kernel<true>, grid, dim3(AP_THREADS), lds_bytes, (hipStream_t)stream, (const uint8_t*)src, src_bytes, desc, table, first,
                           P, Q, taps, tile, win_cap, out, ld_out, out_rows, Lout);
    else
        hipLaunchKernelGGL(audio_resample_kernel<false>, grid, dim3(AP_THREADS), lds_bytes, (hipStream_t)stream, (const uint8_t*)src, src_bytes, desc, table, first,
                           P, Q, taps, tile, win_cap, out, ld_out, out_rows, Lout);
    SC_LAUNCH_CHECK();
    return 0;
}
