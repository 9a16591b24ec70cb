// engine_init.h -- part of engine.hip (one translation unit: the kernels inline into their launchers): weights -> HBM (quantised as stored, exact integer planes, or expanded), every buffer of a context, staging, sync.
// Included by engine.hip behind the definition of umx_hip_ctx; not a stand-alone header.
// ---------------------------------------------------------------- weights
namespace
{
// model.cpp:578-665: q*scale+offset in fp32; F32 passes through
bool dequant(const umx_tensor_view &tv, size_t expect, std::vector<float> &out)
{
    size_t nel = 1;
    for (int i = 0; i < tv.n_dims; ++i)
        nel *= (size_t)tv.ne[i];
    if (nel != expect)
        return false;
    out.resize(nel);
    if (tv.dtype == UMX_DTYPE_F32)
        memcpy(out.data(), tv.data, nel * sizeof(float));
    else if (tv.dtype == UMX_DTYPE_U8)
    {
        const uint8_t *q = static_cast<const uint8_t *>(tv.data);
        for (size_t i = 0; i < nel; ++i)
            out[i] = (float)q[i] * tv.scale + tv.offset;
    }
    else if (tv.dtype == UMX_DTYPE_U16)
    {
        const uint16_t *q = static_cast<const uint16_t *>(tv.data);
        for (size_t i = 0; i < nel; ++i)
            out[i] = (float)q[i] * tv.scale + tv.offset;
    }
    else
        return false;
    return true;
}
} // namespace

int umx_hip_ctx::init(int device_, int hidden, int segment_samples, const umx_tensor_view *tensors, int n_tensors,
                      unsigned create_flags, int n_tracks)
{
    if (n_tracks < 1 || n_tracks > LSTMB_MAX_TRACKS)
    {
        set_error("n_tracks must be in [1, 64]");
        return UMX_ERR_ARG;
    }
    B = n_tracks;
    lstm_batched = B > 1 || (create_flags & UMX_CREATE_LSTM_BATCHED);
    u8_dequant = create_flags & UMX_CREATE_U8_DEQUANT;
    if (hidden <= 0 || hidden % 128 != 0 || hidden > 2048)
    {
        set_error("hidden_size must be a positive multiple of 128 (<= 2048)");
        return UMX_ERR_ARG;
    }
    if (segment_samples < NFFT || segment_samples / HOP + 2 > 4096)
    {
        set_error("segment_samples must be in [4096, 4,193,279] (at most 4095 STFT frames per segment)");
        return UMX_ERR_ARG;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    {
        set_error("no HIP device available (this engine has no CPU fallback)");
        return UMX_ERR_NODEVICE;
    }
    if (device_ < 0 || device_ >= ndev)
    {
        set_error("device index out of range");
        return UMX_ERR_ARG;
    }
    device = device_;
    UMX_HIP_CHECK(hipSetDevice(device));
    H = hidden;
    Hl = H / 2;
    S = Hl / LSTM_UNITS_PER_WG;
    N = segment_samples;
    T = N / HOP + 1; // dsp.hpp:48
    // rows per track lane of the lane-contiguous activation buffers.  Plane GEMMs run over all lanes at once and their
    // tiles may straddle lanes, so lanes follow each other without padding (T rows; 8 % fewer tile rows than lanes padded
    // to the 256-row tile) and only the END of a launch is padded to a tile (Mpad rows of slack in every buffer);
    // the per-lane GEMM flavours launch M = Tp per lane and need whole 128-row tiles.
    Tp = T; // provisional: fixed below once the GEMM flavour is known
    nbatch = (T + WIENER_BATCH - 1) / WIENER_BATCH;

    // ---- index the tensor views by (target, name)
    std::map<std::string, const umx_tensor_view *> idx[4];
    for (int i = 0; i < n_tensors; ++i)
    {
        if (tensors[i].target < 0 || tensors[i].target > 3 || !tensors[i].name || !tensors[i].data)
        {
            set_error("tensor view with bad target / name / data");
            return UMX_ERR_MODEL;
        }
        idx[tensors[i].target][tensors[i].name] = &tensors[i];
    }
    auto get = [&](int tg, const std::string &name, size_t expect, std::vector<float> &out) -> bool {
        auto it = idx[tg].find(name);
        if (it == idx[tg].end())
        {
            set_error("missing tensor '" + name + "' for target " + std::to_string(tg));
            return false;
        }
        if (!dequant(*it->second, expect, out))
        {
            set_error("tensor '" + name + "' has wrong size in model (target " + std::to_string(tg) + ")");
            return false;
        }
        return true;
    };

    const bool keepq = !(create_flags & UMX_CREATE_DEQUANTISE_AT_LOAD); // u8/u16 views stay as they are (config 5)
    auto view = [&](int tg, const std::string &name) -> const umx_tensor_view * {
        auto it = idx[tg].find(name);
        return it == idx[tg].end() ? nullptr : it->second;
    };
    // A GEMM launch covers all four targets with ONE kernel instantiation (its B-operand type is a template
    // parameter), so a matrix stays quantised only if it is stored that way for EVERY target; otherwise it is expanded
    // for all of them.
    auto all_q = [&](const std::string &name, int dtype, size_t expect) {
        for (int tg = 0; tg < 4; ++tg)
        {
            const umx_tensor_view *tv = view(tg, name);
            size_t n = 1;
            for (int i = 0; tv && i < tv->n_dims; ++i)
                n *= (size_t)tv->ne[i];
            if (!keepq || !tv || tv->dtype != dtype || n != expect)
                return false;
        }
        return true;
    };

    if (create_flags & UMX_CREATE_GEMM_F32)
    {
        set_error("UMX_CREATE_GEMM_F32: the fp32-MFMA GEMM flavour was removed in round 3 (slower and, against float64, less accurate "
                  "than the split-operand kernels: profiles/r02_accuracy_vs_float64.txt)");
        return UMX_ERR_ARG;
    }
    // Track-batched contexts fuse the Wiener filter with the inverse STFT (wiener_istft.h: one 1024-thread, 136 KB-LDS
    // workgroup per frame); the single-track context keeps the small kernels, which run beside the other slot's LSTM
    // grids (measured: fused 7.85 ms per segment in the pipeline, unfused 7.41).  UMX_WIENER = fused | stats4 | unfused.
    if (const char *e = getenv("UMX_GEMM_PP"))
        env_gemm_pp = atoi(e);
    if (const char *e = getenv("UMX_GEMM_PS"))
        env_gemm_ps = atoi(e);
    if (const char *e = getenv("UMX_LSTM8_POLL_DELAY")) // tuning: x64 cycles between a wave's publication and its first poll (lstm_batch8.h)
        lstm8_poll_delay = atoi(e);
    if (const char *e = getenv("UMX_LSTM8_PAIRED"))
        env_lstm8_paired = atoi(e) != 0;
    if (const char *e = getenv("UMX_LSTM8_MIN_LANES")) // contexts of this many lanes or more (up to 32) run lstm_batch8_kernel; 99: never
        env_lstm8_min = atoi(e);
    if (const char *e = getenv("UMX_LSTM_POLL_DELAY")) // tuning: x64 cycles a dot wave of the one-track recurrence sleeps before its first poll
        lstm_poll_delay = atoi(e);
    wiener_fused = lstm_batched;
    if (const char *e = getenv("UMX_WIENER")) // fused | stats4 (= statistics kernel + separate filter and inverse-STFT kernels)
        wiener_fused = std::string(e) == "fused";
    // gemm_planes.h for track-batched contexts (large tiles over all lanes); gemm_bf16x3.h for the single-track,
    // latency-optimised context, whose pipeline overlaps small GEMM blocks with two co-resident LSTM grids (the register
    // and LDS budget of DESIGN 4.2 was tuned for exactly that kernel).  Either can be forced.
    gemm_planes = (create_flags & UMX_CREATE_GEMM_PLANES) || (lstm_batched && !(create_flags & UMX_CREATE_GEMM_STAGED));
    Tp = gemm_planes ? std::max(T, 256) : round_up(T, 128); // (a tile must not hold rows of more than two lanes)

    // ---- the GEMM weights
    const int G = 4 * Hl; // gate rows per direction
    // gate rows interleaved so that a workgroup's 64 columns (g,u) are contiguous: PyTorch gate row (i|f|g|o blocks) -> row
    std::vector<int> gate_row(G);
    for (int sl = 0; sl < S; ++sl)
        for (int g = 0; g < 4; ++g)
            for (int u = 0; u < 16; ++u)
                gate_row[g * Hl + sl * 16 + u] = sl * 64 + u * 4 + g; // the 4 gates of a unit share a DPP quad
    // fc3's output rows in the column layout of the mask planes: channel c's 2049 rows at [c * MAGP, ...), zero rows between
    std::vector<int> fc3_row(NOUT);
    for (int r = 0; r < NOUT; ++r)
        fc3_row[r] = r / NBINS * MAGP + r % NBINS;
    // Each weight: its source tensors (W_ih: forward, then reverse, stacked into one matrix), rows x cols of each, the
    // dst_rows x cols_pad block each fills in the device matrix, the destination row of each source row (nullptr: the same
    // row) and the integer type it may stay in.  Rows that none maps to and columns past cols are zero (q = 0 while integer:
    // any finite weight is fine there, padded K columns meet zero activations and padded N rows are never stored).
    struct WeightDesc
    {
        std::string name[2];
        int nsrc, rows, cols, dst_rows, cols_pad;
        const std::vector<int> *dst_row;
        int dtype;
    };
    WeightDesc wd[W_COUNT];
    wd[W_FC1] = {{"fc1.weight"}, 1, H, NIN, H, KX, nullptr, UMX_DTYPE_U8};
    for (int l = 0; l < 3; ++l)
        wd[W_IH0 + l] = {{"lstm.weight_ih_l" + std::to_string(l), "lstm.weight_ih_l" + std::to_string(l) + "_reverse"}, 2, G, H, G, H, &gate_row,
                         UMX_DTYPE_U8};
    wd[W_FC2] = {{"fc2.weight"}, 1, H, 2 * H, H, 2 * H, nullptr, UMX_DTYPE_U16};
    wd[W_FC3] = {{"fc3.weight"}, 1, NOUT, H, NOUT_PAD, H, &fc3_row, UMX_DTYPE_U16};
    auto upload_weight = [&](GemmWeight &w, const void *host, size_t bytes) -> int {
        unsigned char *p = nullptr;
        if (int rc = dalloc(&p, bytes, false))
            return rc;
        UMX_HIP_CHECK(hipMemcpy(p, host, bytes, hipMemcpyHostToDevice));
        w.p = p;
        weight_bytes += bytes;
        return UMX_OK;
    };
    // Weight d of target tg in the form of the context's GEMM flavour (GemmWeight).  Integers as the file holds them if all
    // four targets do: the file's bytes (staged), or exact planes of q - c, c per source tensor (plane flavour, unless
    // UMX_CREATE_U8_DEQUANT; quant_planes.h).
    // Otherwise dequantised fp32: two split planes of w * 2^e, 2^e bringing the source tensor's largest finite |w| into
    // [2^14, 2^15) (plane flavour), or three bf16 planes (staged).
    const bool exact_ok = keepq && !u8_dequant;
    auto load_weight = [&](int tg, const WeightDesc &d, GemmWeight &w) -> int {
        const size_t n = (size_t)d.nsrc * d.dst_rows * d.cols_pad; // elements of one plane
        auto dst = [&](int s, int r) { return ((size_t)s * d.dst_rows + (d.dst_row ? (*d.dst_row)[r] : r)) * d.cols_pad; };
        bool q = true;
        for (int s = 0; s < d.nsrc; ++s)
            q = q && all_q(d.name[s], d.dtype, (size_t)d.rows * d.cols);
        std::vector<unsigned short> planes;
        if (q && (!gemm_planes || exact_ok))
        {
            const size_t esz = d.dtype == UMX_DTYPE_U8 ? 1 : 2;
            if (gemm_planes)
            {
                // u8: q - c in one plane.  u16: q - c as fp16 + exact remainder.  c is each source tensor's own centre and goes into
                // the offset: the kernels take (scale, offset + c scale).  Rows that no source row maps to and columns past cols
                // stay plane value 0.
                w.form = (int)esz;
                planes.assign(w.form * n, 0);
                for (int s = 0; s < d.nsrc; ++s)
                {
                    const umx_tensor_view *tv = view(tg, d.name[s]);
                    unsigned short *hi = planes.data() + (size_t)s * d.dst_rows * d.cols_pad;
                    const QuantCentre qc = quant_planes(tv->data, (int)esz, d.rows, d.cols, d.dst_row ? d.dst_row->data() : nullptr, (size_t)d.cols_pad,
                                                        tv->scale, tv->offset, hi, esz == 2 ? hi + n : nullptr);
                    w.s[s] = tv->scale;
                    w.o[s] = qc.o2;
                }
                return upload_weight(w, planes.data(), planes.size() * sizeof(unsigned short));
            }
            std::vector<unsigned char> qh(n * esz, 0);
            for (int s = 0; s < d.nsrc; ++s)
            {
                const umx_tensor_view *tv = view(tg, d.name[s]);
                for (int r = 0; r < d.rows; ++r)
                    memcpy(&qh[dst(s, r) * esz], static_cast<const unsigned char *>(tv->data) + (size_t)r * d.cols * esz, (size_t)d.cols * esz);
                w.s[s] = tv->scale;
                w.o[s] = tv->offset;
            }
            // the u8 one-plane form of gemm_bf16x3.h: the centre of each source tensor and offset + c scale (quant_planes.h)
            for (int s = 0; s < d.nsrc && esz == 1; ++s)
            {
                const QuantCentre qc = quant_centre(w.s[s], w.o[s]);
                w.c[s] = (float)qc.c;
                w.o2[s] = qc.o2;
            }
            w.form = esz == 1 ? BQ_U8 : BQ_U16;
            return upload_weight(w, qh.data(), qh.size());
        }
        std::vector<float> f(n, 0.f), v;
        if (gemm_planes)
            planes.assign(2 * n, 0);
        for (int s = 0; s < d.nsrc; ++s)
        {
            if (!get(tg, d.name[s], (size_t)d.rows * d.cols, v))
                return UMX_ERR_MODEL;
            for (int r = 0; r < d.rows; ++r)
                memcpy(&f[dst(s, r)], &v[(size_t)r * d.cols], sizeof(float) * d.cols);
            if (gemm_planes)
            {
                float mx = 0.f, scale = 1.f;
                for (float x : v)
                    if (std::isfinite(x))
                        mx = std::max(mx, std::fabs(x));
                if (mx > 0.f)
                {
                    int x;
                    (void)std::frexp(mx, &x);
                    const int e = std::min(std::max(GP_SPLIT_FIXED_EXP + 1 - x, -100), 100);
                    scale = std::ldexp(1.0f, e);
                    w.s[s] = std::ldexp(1.0f, -e);
                }
                const size_t b0 = (size_t)s * d.dst_rows * d.cols_pad;
                for (size_t i = b0; i < b0 + (size_t)d.dst_rows * d.cols_pad; ++i)
                    f16_split(f[i] * scale, &planes[i], &planes[n + i]);
            }
        }
        if (gemm_planes)
            w.form = 2;
        else
        {
            w.form = BQ_F32;
            planes.resize(3 * n);
            for (size_t i = 0; i < n; ++i)
                split3_host(f[i], planes[i], planes[n + i], planes[2 * n + i]);
        }
        return upload_weight(w, planes.data(), planes.size() * sizeof(unsigned short));
    };

    std::vector<float> whh_h[3], bhh_h[3];
    std::vector<unsigned char> whh_qh[3];
    bool whh_all_u8 = true;
    for (int l = 0; l < 3; ++l)
        for (int dir = 0; dir < 2; ++dir)
            whh_all_u8 = whh_all_u8 && all_q("lstm.weight_hh_l" + std::to_string(l) + (dir ? "_reverse" : ""), UMX_DTYPE_U8, (size_t)G * Hl);
    if (whh_all_u8)
        for (int l = 0; l < 3; ++l)
            whh_qh[l].assign((size_t)8 * S * Hl * 64, 0);
    for (int l = 0; l < 3; ++l)
    {
        whh_h[l].assign((size_t)8 * S * Hl * 64, 0.f);
        bhh_h[l].assign((size_t)8 * S * 64, 0.f);
    }
    for (int tg = 0; tg < 4; ++tg)
    {
        TargetBufs &b = tb[tg];
        std::vector<float> v, w;
        // input / output scaling, duplicated per channel like model.cpp:240-290
        if (!get(tg, "input_scale", CROP, v))
            return UMX_ERR_MODEL;
        w.assign(KX, 0.f);
        for (int k = 0; k < NIN; ++k)
            w[k] = v[k % CROP];
        if (int rc = upload(&b.in_scale, w))
            return rc;
        if (!get(tg, "input_mean", CROP, v))
            return UMX_ERR_MODEL;
        w.assign(KX, 0.f);
        for (int k = 0; k < NIN; ++k)
            w[k] = v[k % CROP];
        if (int rc = upload(&b.in_mean, w))
            return rc;
        if (!get(tg, "output_scale", NBINS, v))
            return UMX_ERR_MODEL;
        // fc3's columns: channel c at [c * MAGP, c * MAGP + 2049) (gemm_common.h); model.cpp:240-290 duplicates per channel
        w.assign(NOUT_PAD, 0.f);
        for (int c = 0; c < 2; ++c)
            for (int k = 0; k < NBINS; ++k)
                w[c * MAGP + k] = v[k];
        if (int rc = upload(&b.out_scale, w))
            return rc;
        if (!get(tg, "output_mean", NBINS, v))
            return UMX_ERR_MODEL;
        w.assign(NOUT_PAD, 0.f);
        for (int c = 0; c < 2; ++c)
            for (int k = 0; k < NBINS; ++k)
                w[c * MAGP + k] = v[k];
        if (int rc = upload(&b.out_mean, w))
            return rc;
        if (int rc = load_weight(tg, wd[W_FC1], b.w[W_FC1]))
            return rc;
        const char *bnn[4] = {"running_mean", "running_var", "weight", "bias"};
        for (int k = 0; k < 4; ++k)
        {
            if (!get(tg, std::string("bn1.") + bnn[k], H, v))
                return UMX_ERR_MODEL;
            if (int rc = upload(&b.bn1[k], v))
                return rc;
            if (!get(tg, std::string("bn2.") + bnn[k], H, v))
                return UMX_ERR_MODEL;
            if (int rc = upload(&b.bn2[k], v))
                return rc;
            if (!get(tg, std::string("bn3.") + bnn[k], NOUT, v))
                return UMX_ERR_MODEL;
            w.assign(NOUT_PAD, k == 1 ? 1.f : 0.f); // padded running_var = 1: no 0/0 in dead columns
            for (int c = 0; c < 2; ++c)
                memcpy(&w[c * MAGP], &v[c * NBINS], sizeof(float) * NBINS);
            if (int rc = upload(&b.bn3[k], w))
                return rc;
        }
        if (int rc = load_weight(tg, wd[W_FC2], b.w[W_FC2]))
            return rc;
        if (int rc = load_weight(tg, wd[W_FC3], b.w[W_FC3]))
            return rc;
        for (int l = 0; l < 3; ++l)
        {
            if (int rc = load_weight(tg, wd[W_IH0 + l], b.w[W_IH0 + l]))
                return rc;
            // biases and W_hh: the gate rows of W_ih; W_hh per workgroup slice [chain][S][Hl][64]
            std::vector<float> ihb((size_t)2 * G);
            for (int dir = 0; dir < 2; ++dir)
            {
                const std::string sfx = "_l" + std::to_string(l) + (dir ? "_reverse" : "");
                std::vector<float> whhv, bih, bhhv;
                if ((!whh_all_u8 && !get(tg, "lstm.weight_hh" + sfx, (size_t)G * Hl, whhv)) ||
                    !get(tg, "lstm.bias_ih" + sfx, G, bih) || !get(tg, "lstm.bias_hh" + sfx, G, bhhv))
                    return UMX_ERR_MODEL;
                const int chain = tg * 2 + dir;
                const umx_tensor_view *hhv = view(tg, "lstm.weight_hh" + sfx);
                const unsigned char *hhq = whh_all_u8 ? static_cast<const unsigned char *>(hhv->data) : nullptr;
                if (whh_all_u8)
                {
                    whh_s[l][chain] = hhv->scale;
                    whh_o[l][chain] = hhv->offset;
                }
                for (int row = 0; row < G; ++row)
                {
                    const int sl = gate_row[row] / 64, col = gate_row[row] % 64;
                    ihb[(size_t)dir * G + gate_row[row]] = bih[row];
                    bhh_h[l][((size_t)chain * S + sl) * 64 + col] = bhhv[row];
                    for (int k = 0; k < Hl; ++k)
                    {
                        const size_t di = (((size_t)chain * S + sl) * Hl + k) * 64 + col;
                        if (whh_all_u8)
                            whh_qh[l][di] = hhq[(size_t)row * Hl + k];
                        else
                            whh_h[l][di] = whhv[(size_t)row * Hl + k];
                    }
                }
            }
            if (int rc = upload(&b.ih_b[l], ihb))
                return rc;
        }
    }
    for (int l = 0; l < 3; ++l)
    {
        if (whh_all_u8)
        {
            if (int rc = upload(&whh_q[l], whh_qh[l]))
                return rc;
            weight_bytes += whh_qh[l].size();
        }
        else
        {
            if (int rc = upload(&whh[l], whh_h[l]))
                return rc;
            weight_bytes += whh_h[l].size() * sizeof(float);
        }
        if (int rc = upload(&bhh[l], bhh_h[l]))
            return rc;
    }
    // ---- tables: window (dsp.hpp:61-78, the reference's float PI), window sum-square
    // (dsp.hpp:80-101, same accumulation order), FFT twiddles (rounded from double)
    {
        std::vector<float> w(NFFT);
        static const float PI = 3.14159265359F;
        const float floatN = (float)(NFFT + 1);
        for (int n = 0; n < NFFT; ++n)
            w[n] = 0.5F * (1.0F - cosf(2.0F * PI * (float)n / (floatN - 1)));
        if (int rc = upload(&window, w))
            return rc;
        const size_t total = (size_t)NFFT + (size_t)HOP * (T - 1);
        std::vector<float> nwh(total, 0.f);
        for (int i = 0; i < T; ++i)
        {
            const size_t s0 = (size_t)i * HOP;
            for (size_t j = s0; j < std::min(total, s0 + NFFT); ++j)
                nwh[j] += w[j - s0] * w[j - s0];
        }
        if (int rc = upload(&nw, nwh))
            return rc;
        std::vector<float2> t1(256), t2(4096);
        for (int r = 0; r < 16; ++r)
            for (int k = 0; k < 16; ++k)
            {
                const double ph = -2.0 * M_PI * (double)(r * k) / 256.0;
                t1[r * 16 + k] = make_float2((float)cos(ph), (float)sin(ph));
            }
        for (int r = 0; r < 16; ++r)
            for (int j = 0; j < 256; ++j)
            {
                const double ph = -2.0 * M_PI * (double)(r * j) / 4096.0;
                t2[r * 256 + j] = make_float2((float)cos(ph), (float)sin(ph));
            }
        if (int rc = upload(&tw1, t1))
            return rc;
        if (int rc = upload(&tw2, t2))
            return rc;
    }
    // ---- per-segment buffers: two pipeline slots x B track lanes
    if (int rc = dalloc(&audio_in, (size_t)2 * N))
        return rc;
    for (int k = 0; k < 4; ++k)
        if (int rc = dalloc(&out_dev[k], (size_t)2 * N))
            return rc;
    if (int rc = dalloc(&state, state_floats() * B))
        return rc;
    if (int rc = dalloc(&state_alt, state_floats() * B))
        return rc;
    if (int rc = dalloc(&backup, (size_t)kBackupCalls * 3 * state_floats() * B))
        return rc;
    lsync_words = LSTM_SYNC_HEADER_WORDS + std::max(granule_count(S) * 2, lstm_batched ? lstmb_granule_words(Hl) * ((B + LSTMB_GROUP_TRACKS - 1) / LSTMB_GROUP_TRACKS) : (size_t)0);
    // Two slots.  (Three were tried for single-track contexts in round 3 -- a third segment in flight has its front stage
    // done by the time an LSTM grid retires, so that two grids would be resident all the time: 7.57 ms per segment against
    // 6.70 with two; the grids and the GEMM blocks beside them only slow each other down, avg LSTM launch 3.03 -> 3.79 ms.)
    nslots = 2;
    if (gemm_planes)
    {
        // the plane GEMMs address their operands and fc3's mask output through buffer resources with 32-bit byte offsets
        // (gemm_planes.h: both planes of an operand behind one base; gemm_common.h: all lanes' masks behind one base): refuse
        // lane x segment-length combinations that do not fit instead of reading zeros past the range check
        const unsigned long long rows = (unsigned long long)B * Tp + Mpad;
        const unsigned long long planes_bytes = 2ull * rows * (unsigned long long)std::max(KX, 2 * H) * 2ull;
        const unsigned long long mask_bytes = (unsigned long long)B * 2ull * T * MAGP * 4ull;
        if (planes_bytes >= (1ull << 31) || mask_bytes >= (1ull << 32))
        {
            set_error("track lanes x segment length exceed the 32-bit addressing of the plane GEMMs' operands: fewer lanes or a shorter segment");
            return UMX_ERR_ARG;
        }
    }
    for (int si = 0; si < nslots; ++si)
    {
        Slot &sl = slot[si];
        UMX_HIP_CHECK(hipStreamCreateWithFlags(&sl.stream, hipStreamNonBlocking));
        // Buffers that a launch covering several track lanes reads or writes (the batched LSTM kernel, the plane GEMMs
        // with M = lanes x Tp) are ONE allocation per slot (and target), lane after lane at a constant stride.
        float *x_all = nullptr;
        if (int rc = dalloc(&x_all, ((size_t)B * Tp + Mpad) * KX))
            return rc;
        for (int tg = 0; tg < 4; ++tg)
        {
            float *cat_all = nullptr, *la_all = nullptr, *lb_all = nullptr, *P_all = nullptr, *a2_all = nullptr, *mag_all = nullptr;
            if (int rc = dalloc(&cat_all, ((size_t)B * Tp + Mpad) * 2 * H))
                return rc;
            if (int rc = dalloc(&la_all, ((size_t)B * Tp + Mpad) * H))
                return rc;
            if (int rc = dalloc(&lb_all, ((size_t)B * Tp + Mpad) * H))
                return rc;
            if (int rc = dalloc(&P_all, ((size_t)B * Tp + Mpad) * 4 * H))
                return rc;
            if (int rc = dalloc(&a2_all, ((size_t)B * Tp + Mpad) * H))
                return rc;
            if (int rc = dalloc(&mag_all, (size_t)B * 2 * T * MAGP))
                return rc;
            unsigned short *xs_p = nullptr, *cat_p = nullptr, *la_p = nullptr, *lb_p = nullptr, *a2_p = nullptr;
            float *rs[8] = {};
            if (gemm_planes) // planes [2][B * Tp][K]: plane-major over ALL lanes, so that M runs across the lanes
            {
                if (int rc = dalloc(&xs_p, 2 * ((size_t)B * Tp + Mpad) * KX))
                    return rc;
                if (int rc = dalloc(&cat_p, 2 * ((size_t)B * Tp + Mpad) * 2 * H))
                    return rc;
                for (unsigned short **q : {&la_p, &lb_p, &a2_p})
                    if (int rc = dalloc(q, 2 * ((size_t)B * Tp + Mpad) * H))
                        return rc;
                for (int k = 0; k < 8; ++k) // [2..4]: the recurrence's outputs, one array per direction when it writes the planes itself
                    if (int rc = dalloc(&rs[k], ((size_t)B * Tp + Mpad) * (k >= 2 && k <= 4 ? 2 : 1)))
                        return rc;
            }
            for (int ln = 0; ln < B; ++ln)
            {
                TargetAct &b = sl.lane[ln].ta[tg];
                b.cat = cat_all + (size_t)ln * Tp * 2 * H;
                b.la = la_all + (size_t)ln * Tp * H;
                b.lb = lb_all + (size_t)ln * Tp * H;
                b.P = P_all + (size_t)ln * Tp * 4 * H;
                b.a2 = a2_all + (size_t)ln * Tp * H;
                b.mag = mag_all + (size_t)ln * 2 * T * MAGP;
                if (gemm_planes) // lane ln's rows start at row ln * Tp of every plane
                {
                    b.xs_p = xs_p + (size_t)ln * Tp * KX;
                    b.cat_p = cat_p + (size_t)ln * Tp * 2 * H;
                    b.la_p = la_p + (size_t)ln * Tp * H;
                    b.lb_p = lb_p + (size_t)ln * Tp * H;
                    b.a2_p = a2_p + (size_t)ln * Tp * H;
                    b.rs_xs = rs[0] + (size_t)ln * Tp;
                    b.rs_catL = rs[1] + (size_t)ln * Tp;
                    b.rs_catR = rs[2] + (size_t)ln * Tp;
                    b.rs_la = rs[3] + (size_t)ln * Tp;
                    b.rs_lb = rs[4] + (size_t)ln * Tp;
                    b.rs_a2 = rs[5] + (size_t)ln * Tp;
                    b.rsc_xs = rs[6] + (size_t)ln * Tp;
                    b.rsc_a2 = rs[7] + (size_t)ln * Tp;
                }
            }
        }
        {
            // every lane's streaming buffers a fixed stride apart (lane_strides()): the streaming kernels take lane 0's
            // pointers and cover all active lanes in one launch (common.h LaneSet)
            const WienerStrides ls = lane_strides();
            float2 *spec_all, *y_all, *frames_all;
            float *wpart_all, *Rc_all;
            unsigned *maxabs_all;
            if (int rc = dalloc(&spec_all, (size_t)B * ls.spec))
                return rc;
            if (int rc = dalloc(&y_all, (size_t)B * ls.y))
                return rc;
            if (int rc = dalloc(&frames_all, (size_t)B * ls.frames))
                return rc;
            if (int rc = dalloc(&wpart_all, (size_t)B * ls.part))
                return rc;
            if (int rc = dalloc(&Rc_all, (size_t)B * ls.rc))
                return rc;
            if (int rc = dalloc(&maxabs_all, (size_t)B))
                return rc;
            for (int ln = 0; ln < B; ++ln)
            {
                Lane &L = sl.lane[ln];
                L.x = x_all + (size_t)ln * Tp * KX;
                L.spec = spec_all + (size_t)ln * ls.spec;
                L.y = y_all + (size_t)ln * ls.y;
                L.frames = frames_all + (size_t)ln * ls.frames;
                L.wpart = wpart_all + (size_t)ln * ls.part;
                L.Rc = Rc_all + (size_t)ln * ls.rc;
                L.maxabs = maxabs_all + ln;
            }
        }
        if (int rc = dalloc(&sl.status, 4))
            return rc;
        if (int rc = dalloc(&sl.hbuf, (size_t)2 * 8 * Hl))
            return rc;
        if (int rc = dalloc(&sl.lsync, lsync_words))
            return rc;
        if (int rc = dalloc(&sl.lprof, 1024 + 64 * 8 * 5))
            return rc;
        for (int i = 0; i <= ST_COUNT; ++i)
            UMX_HIP_CHECK(hipEventCreate(&sl.ev[i]));
        for (int i : {ST_FC1, ST_IH0, ST_IH1, ST_IH2, ST_FC2, ST_FC3})
            UMX_HIP_CHECK(hipEventCreate(&sl.evk[i]));
        for (int l = 0; l < 3; ++l)
            UMX_HIP_CHECK(hipEventCreateWithFlags(&sl.rec_done[l], hipEventDisableTiming));
    }
    stream = slot[0].stream;
    {
        // Residency of the recurrences, from the LSTM kernel table: the smallest occupancy over the entries of a family at this
        // hidden size (both activation flavours, fp32- and u8-resident W_hh, one and two octets per workgroup), each with its LDS
        // limit raised.  The one-track persistent kernel: the two-grid co-residency of the pipeline rests on it.  lstm_batch_kernel:
        // at the LDS a launch of all of this context's lanes (at most a group of 16) asks for.
        // lstm_batch8_kernel (octets of 8 lanes x column shards of 64 units, lstm_batch8.h): LSTM hidden 512 / 256 with the u8-resident
        // W_hh, chosen per CONTEXT and used for every launch of it -- its sums are not the bits of lstm_batch_kernel, and a lane's
        // result must not depend on who rides along.  Everything else (hidden 256 / 128, fp32-resident W_hh, UMX_LSTM8_MIN_LANES=99)
        // runs lstm_batch_kernel, a group of 16 lanes per launch, the groups one after the other.
        int cus = 0;
        UMX_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
        n_cus = cus;
        const bool want8 = lstm_batched && B >= env_lstm8_min && !u8_dequant && whh_q[0] && whh_q[1] && whh_q[2];
        const LstmbLanes ll = lstmb_lanes(B);
        constexpr int kNone = 1 << 30;
        int per_cu[3] = {kNone, kNone, kNone}; // by family
        for (const LstmKernel &k : kLstmKernels)
        {
            if (k.hl != Hl || (k.family == LSTM_BATCH && !lstm_batched) || (k.family == LSTM_BATCH8 && !want8))
                continue;
            if (k.lds)
                UMX_HIP_CHECK(hipFuncSetAttribute(k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)k.lds));
            int v = 0;
            UMX_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&v, k.fn, LSTM_THREADS, k.family == LSTM_BATCH ? lstmb_lds_bytes(ll.nbp, ll.bulk) : k.lds));
            per_cu[k.family] = std::min(per_cu[k.family], v);
        }
        lstm_capacity = per_cu[LSTM_PERSISTENT] == kNone ? 0 : per_cu[LSTM_PERSISTENT] * cus; // (no kernel: the per-step driver)
        if (lstm_batched)
        {
            if (per_cu[LSTM_BATCH] == kNone)
            {
                set_error("track batching needs hidden_size in " + lstm_hidden_sizes(LSTM_BATCH));
                return UMX_ERR_ARG;
            }
            lstm_batch8_ok = per_cu[LSTM_BATCH8] != kNone && per_cu[LSTM_BATCH8] >= 1 && 8 * 32 <= per_cu[LSTM_BATCH8] * cus;
            if (lstm_batch8_ok)
            {
                // lstm_batch8_kernel addresses its streams through buffer resources with 32-bit offsets (lstm_batch8.h): the rows of W_ih x,
                // which it only loads, up to 2^32 bytes per target; the fp32 rows and the fused planes, which it stores, below
                // LSTM8_OOR -- the lane offset of a lane with nothing to store, which the range check must drop
                const unsigned long long rows = (unsigned long long)B * Tp + Mpad;
                const unsigned long long p_bytes = (unsigned long long)B * Tp * 4ull * H * 4ull, out_bytes = (unsigned long long)B * Tp * 2ull * H * 4ull;
                const unsigned long long plane_bytes = 2ull * rows * 2ull * H * 2ull;
                const unsigned long long rs_bytes = 2ull * rows * 4ull; // the row sums, [2 dirs][rows]: stored through LSTM8_OOR bytes as well
                if (p_bytes >= (1ull << 32) || out_bytes >= LSTM8_OOR || plane_bytes >= LSTM8_OOR || rs_bytes >= LSTM8_OOR)
                {
                    set_error("track lanes x segment length exceed the 32-bit addressing of the batched recurrence's streams: fewer lanes or a shorter segment");
                    return UMX_ERR_ARG;
                }
            }
            // the persistent launches of a lstm_batch8 context are lstm_batch8_kernel's: its occupancy decides
            lstm_batch_capacity = per_cu[lstm_batch8_ok ? LSTM_BATCH8 : LSTM_BATCH] * cus;
            // the recurrence writes the plane GEMMs' A operands (layers 1, 2 and fc2's right half) and their row sums itself where
            // it runs on the u8-resident W_hh (its gate lanes hold h as two fp16 planes, its all-ones tile the row sums): no
            // split_planes launches for them (lstm_batch.h, LstmBArgs::planes).  -DUMX_FUSE_LSTM_PLANES=0: A/B builds
            lstm_rowsums = UMX_FUSE_LSTM_PLANES && gemm_planes && !u8_dequant && whh_q[0] && whh_q[1] && whh_q[2];
            lstm_writes_planes = lstm_rowsums;
        }
    }
    // dynamic LDS > 64 KiB must be opted into: the fused Wiener kernels (four transforms + the window) and every entry of the
    // GEMM kernel tables
    for (const void *fn : {reinterpret_cast<const void *>(wiener_istft_kernel<true>), reinterpret_cast<const void *>(wiener_istft_kernel<false>),
                           reinterpret_cast<const void *>(wiener_istft_v_kernel)})
        UMX_HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)WI_LDS_BYTES));
    for (int mode = G_FC1; mode <= G_FC3; ++mode)
    {
        std::vector<GemmKernel> ks;
        for (int bq : {BQ_F32, BQ_U8, BQ_U16, BQ_U8X})
            ks.push_back(bx_kernel(mode, bq));
        for (int nbp = 1; nbp <= 2; ++nbp)
            for (int kind = 0; kind < GP_KINDS; ++kind)
                ks.push_back(gp_kernel(mode, nbp, kind));
        for (const GemmKernel &k : ks)
            if (k.fn)
                UMX_HIP_CHECK(hipFuncSetAttribute(k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, k.lds));
    }
    UMX_HIP_CHECK(hipDeviceSynchronize());
    return UMX_OK;
}

int umx_hip_ctx::ensure_staging()
{
    if (stage_in[0])
        return UMX_OK;
    UMX_HIP_CHECK(hipStreamCreateWithFlags(&copy_stream, hipStreamNonBlocking));
    for (int si = 0; si < nslots; ++si)
    {
        for (hipEvent_t *e : {&slot[si].k_done, &slot[si].out_free})
            UMX_HIP_CHECK(hipEventCreateWithFlags(e, hipEventDisableTiming));
        if (int rc = dalloc(&stage_in[si], (size_t)2 * N * B, false))
            return rc;
        for (int k = 0; k < 4 * B; ++k)
            if (int rc = dalloc(&stage_out[si][k], (size_t)2 * N, false))
                return rc;
    }
    return UMX_OK;
}

// Host-pointer calls: where the stems of call k go out (round 3; kernel + copy timelines by tools/pcie_trace.sh).
//   * On the slot's own stream right behind its kernels (rounds 1-2), the download (48 ms for 32 lanes) stands in front of
//     call k + 2's upload and kernels; the two slots then fall into lock step -- kernels of two calls, downloads of two
//     calls, uploads of two calls, nothing overlapping: 128 ms per step against 78 ms of kernels.
//   * On the slot's own stream one call LATER (behind call k + 2's front stage): the same 129 ms.
//   * On the OTHER slot's stream behind call k + 1's kernels: 110-113 ms (the copies stay on the DMA engines, but a call's
//     kernels end at about the same time as the next call's, so the download still starts late).
//   * On a copy stream of its own behind an event (this code): 91-93 ms.  The runtime executes these copies as shader blits
//     (a download that does not follow kernels of its own stream), which wait for compute units behind the persistent LSTM
//     grids; a marker kernel in front of them does not change that.
// A separate UPLOAD stream as well made everything serial (141 ms): streams beyond the runtime's hardware queues share one.
int umx_hip_ctx::queue_download(const DeferredDownload &d, hipStream_t on)
{
    Slot &src = slot[d.si];
    if (on != src.stream)
        UMX_HIP_CHECK(hipStreamWaitEvent(on, src.k_done, 0));
    for (int ln = 0; ln < d.nb; ++ln)
        if (d.n[ln] > 0)
            for (int s2 = 0; s2 < 4; ++s2)
                UMX_HIP_CHECK(hipMemcpyAsync(d.host[4 * ln + s2], stage_out[d.si][4 * ln + s2], sizeof(float) * 2 * (size_t)d.n[ln],
                                             hipMemcpyDeviceToHost, on));
    UMX_HIP_CHECK(hipEventRecord(src.out_free, on));
    src.out_free_valid = true;
    return UMX_OK;
}

int umx_hip_ctx::sync_all()
{
    for (int si = 0; si < nslots; ++si)
        UMX_HIP_CHECK(hipStreamSynchronize(slot[si].stream));
    if (copy_stream)
        UMX_HIP_CHECK(hipStreamSynchronize(copy_stream));
    for (int si = 0; si < nslots; ++si)
        slot[si].out_free_valid = false; // drained
    return UMX_OK;
}
