// torch.ops.dbsr.* -- the reference's functional sub-seams as PyTorch operators (one
// shared object loaded with torch.ops.load_library, TORCH_LIBRARY(dbsr, m) schemas with a HIP-device
// implementation).  Each op validates its inputs like the reference (TORCH_CHECK on device, dtype,
// contiguity: correlation.py:286-287), lays the NCHW tensors out channels-last for the C ABI of
// libdbsr_hip.so (include/dbsr_hip.h), launches on the current HIP stream and returns NCHW tensors.
//
//   dbsr::correlation(first, second, leaky)        external/pwcnet/correlation/correlation.py:278-330,385
//   dbsr::correlation_backward(...)                correlation.py:332-383 (K3/K4)
//   dbsr::backwarp(input, flow)                    models/alignment/pwcnet.py:16-38
//   dbsr::warp_bilinear(feat, flow)                models/layers/warp.py:19-46
//   dbsr::warp_bilinear_backward(grad, flow)       (grid_sample backward w.r.t. the features)
//   dbsr::warp_bilinear_flow_backward(grad, feat, flow)   (grid_sample backward w.r.t. the flow)
//   dbsr::backwarp_backward(grad, input, flow, need_input, need_flow)   (w.r.t. both; the mask takes none)
//   dbsr::fuse_softmax(logits, feats, want_weights) models/dbsr/merging.py:116-126
//   dbsr::fuse_backward(weights, feats, fused, dfused)
//   dbsr::conv2d_fused(x, w, b, stride, padding, dilation, act, residual, post_act)
//                                                  nn.Conv2d + models/layers/blocks.py:46-96 epilogues
//   dbsr::conv2d_backward(grad, x, w, out, stride, padding, dilation, act, need_x, need_w, need_b)
//   dbsr::conv_transpose2d_k4s2(x, w, b) / _backward   nn.ConvTranspose2d(k4, s2, p1), pwcnet.py:119-120
//   dbsr::flow_finalize(flow, H, W) / _backward    pwcnet.py:274-279
//   dbsr::resize_bilinear(x, Hp, Wp)               pwcnet.py:266-271 (forward only)
// Autograd formulas for correlation / backwarp / warp / fusion / the convs are registered from Python (dbsr_amd/torch_ops.py)
// with torch.library.register_autograd on top of the *_backward ops.
#include <ATen/ATen.h>
#include <ATen/hip/HIPContext.h>
#include <torch/library.h>

#include <map>
#include <mutex>
#include <optional>
#include <tuple>
#include <vector>

#include "../../../include/dbsr_hip.h"

namespace {

int dcode(at::ScalarType t) {
    switch (t) {
        case at::kFloat: return DBSR_F32;
        case at::kBFloat16: return DBSR_BF16;
        case at::kHalf: return DBSR_F16;
        default: TORCH_CHECK(false, "dbsr: unsupported dtype ", t, " (float32, bfloat16, float16)");
    }
    return -1;
}

void check(int rc, const char* what) {
    TORCH_CHECK(rc == 0, what, " failed (rc=", rc, "): ", dbsr_last_error());
}

void* cur_stream() { return (void*)at::hip::getCurrentHIPStream().stream(); }

int64_t r8(int64_t c) { return (c + 7) / 8 * 8; }
int64_t conv_ld(int64_t c) { return c <= 16 ? r8(c) : (c + 31) / 32 * 32; }   // dbsr_conv2d channel padding

// [N,C,H,W] -> zero-padded channels-last [N,H,W,ld]
at::Tensor nhwc(const at::Tensor& x, int64_t ld, at::ScalarType dt) {
    auto t = x.permute({0, 2, 3, 1}).to(dt);
    auto out = at::zeros({x.size(0), x.size(2), x.size(3), ld}, x.options().dtype(dt));
    out.narrow(3, 0, x.size(1)).copy_(t);
    return out;
}
at::Tensor nchw(const at::Tensor& y, int64_t c) { return y.narrow(3, 0, c).permute({0, 3, 1, 2}).contiguous(); }

dbsr_tensor desc(const at::Tensor& t, int64_t ld, int64_t c0 = 0, int64_t img_stride = -1, dbsr_frame_map m = {1, 1, 0, 1}) {
    dbsr_tensor d;
    d.ptr = t.data_ptr();
    d.dtype = dcode(t.scalar_type());
    d.img_stride = img_stride >= 0 ? img_stride : (t.dim() > 1 ? t[0].numel() : t.numel());
    d.ld = (int)ld;
    d.c0 = (int)c0;
    d.map = m;
    return d;
}
dbsr_tensor null_desc() {
    dbsr_tensor d{};
    d.map = {1, 1, 0, 1};
    return d;
}

void need_hip(const at::Tensor& t, const char* name) {
    TORCH_CHECK(t.is_cuda(), "dbsr::", name, ": inputs must be on the HIP device (correlation.py:324-325 has no "
                "CPU path either)");
}

// ------------------------------------------------------------------------------------------------
at::Tensor correlation(const at::Tensor& first, const at::Tensor& second, bool leaky) {
    need_hip(first, "correlation");
    TORCH_CHECK(first.is_contiguous() && second.is_contiguous(), "dbsr::correlation: inputs must be contiguous "
                "(correlation.py:286-287)");
    TORCH_CHECK(first.sizes() == second.sizes() && first.dim() == 4, "dbsr::correlation: [N,C,H,W] inputs of equal shape");
    const int64_t N = first.size(0), C = first.size(1), H = first.size(2), W = first.size(3);
    const auto dt = first.scalar_type();
    auto a = nhwc(first, r8(C), dt), b = nhwc(second, r8(C), dt);
    auto out = at::zeros({N, H, W, 88}, first.options());
    check(dbsr_correlation(N, H, W, C, desc(a, r8(C)), desc(b, r8(C)), desc(out, 88), leaky ? 1 : 0, cur_stream()),
          "dbsr_correlation");
    return nchw(out, 81);
}

std::tuple<at::Tensor, at::Tensor> correlation_backward(const at::Tensor& grad, const at::Tensor& first,
                                                        const at::Tensor& second, const at::Tensor& out, bool leaky) {
    need_hip(grad, "correlation_backward");
    const int64_t N = first.size(0), C = first.size(1), H = first.size(2), W = first.size(3);
    const auto dt = first.scalar_type();
    auto a = nhwc(first, r8(C), dt), b = nhwc(second, r8(C), dt);
    auto g = nhwc(grad, 88, dt), o = nhwc(out, 88, dt);
    auto da = at::zeros_like(a), db = at::zeros_like(b);
    check(dbsr_correlation_backward(N, H, W, C, desc(a, r8(C)), desc(b, r8(C)), desc(o, 88), desc(g, 88),
                                    leaky ? 1 : 0, desc(da, r8(C)), desc(db, r8(C)), cur_stream()),
          "dbsr_correlation_backward");
    return {nchw(da, C), nchw(db, C)};
}

at::Tensor backwarp(const at::Tensor& input, const at::Tensor& flow) {
    need_hip(input, "backwarp");
    TORCH_CHECK(input.dim() == 4 && flow.dim() == 4 && flow.size(1) == 2, "dbsr::backwarp: [N,C,H,W] x [N,2,H,W]");
    const int64_t N = input.size(0), C = input.size(1), H = input.size(2), W = input.size(3);
    const auto dt = input.scalar_type();
    auto x = nhwc(input, r8(C), dt);
    auto fl = flow.permute({0, 2, 3, 1}).to(at::kFloat).contiguous();
    auto out = at::zeros_like(x);
    check(dbsr_backwarp(N, H, W, C, desc(x, r8(C)), desc(fl, 2), 1.0f, desc(out, r8(C)), cur_stream()),
          "dbsr_backwarp");
    return nchw(out, C);
}

at::Tensor warp_bilinear(const at::Tensor& feat, const at::Tensor& flow) {
    need_hip(feat, "warp_bilinear");
    TORCH_CHECK(feat.dim() == 4 && flow.dim() == 4 && flow.size(1) == 2, "dbsr::warp_bilinear: [N,C,H,W] x [N,2,H,W]");
    const int64_t N = feat.size(0), C = feat.size(1), H = feat.size(2), W = feat.size(3);
    const auto dt = feat.scalar_type();
    auto x = nhwc(feat, r8(C), dt);
    auto fl = flow.to(at::kFloat).contiguous();
    auto out = at::zeros_like(x);
    check(dbsr_warp_bilinear(N, H, W, r8(C), desc(x, r8(C)), fl.data_ptr<float>(), 2 * H * W, desc(out, r8(C)),
                             cur_stream()),
          "dbsr_warp_bilinear");
    return nchw(out, C);
}

at::Tensor warp_bilinear_backward(const at::Tensor& grad, const at::Tensor& flow) {
    need_hip(grad, "warp_bilinear_backward");
    const int64_t N = grad.size(0), C = grad.size(1), H = grad.size(2), W = grad.size(3);
    auto g = nhwc(grad, r8(C), grad.scalar_type());
    auto fl = flow.to(at::kFloat).contiguous();
    auto out = at::zeros({N, H, W, r8(C)}, grad.options().dtype(at::kFloat));
    check(dbsr_warp_backward(N, H, W, r8(C), desc(g, r8(C)), fl.data_ptr<float>(), 2 * H * W, out.data_ptr<float>(),
                             dbsr_frame_map{1, 1, 0, 1}, H * W * r8(C), cur_stream()),
          "dbsr_warp_backward");
    return nchw(out, C).to(grad.scalar_type());
}

at::Tensor warp_bilinear_flow_backward(const at::Tensor& grad, const at::Tensor& feat, const at::Tensor& flow) {
    need_hip(grad, "warp_bilinear_flow_backward");
    TORCH_CHECK(feat.dim() == 4 && grad.sizes() == feat.sizes() && flow.dim() == 4 && flow.size(1) == 2,
                "dbsr::warp_bilinear_flow_backward: grad / feat [N,C,H,W], flow [N,2,H,W]");
    const int64_t N = feat.size(0), C = feat.size(1), H = feat.size(2), W = feat.size(3);
    const auto dt = feat.scalar_type();
    auto x = nhwc(feat, r8(C), dt), g = nhwc(grad, r8(C), dt);
    auto fl = flow.to(at::kFloat).contiguous();
    auto out = at::empty({N, 2, H, W}, feat.options().dtype(at::kFloat));
    check(dbsr_warp_flow_backward(N, H, W, r8(C), desc(x, r8(C)), desc(g, r8(C)), fl.data_ptr<float>(), 2 * H * W,
                                  out.data_ptr<float>(), 2 * H * W, 0, cur_stream()),
          "dbsr_warp_flow_backward");
    return out.to(flow.scalar_type());
}

// (an unwanted gradient is returned as an empty tensor and is not computed)
std::tuple<at::Tensor, at::Tensor> backwarp_backward(const at::Tensor& grad, const at::Tensor& input,
                                                     const at::Tensor& flow, bool need_input, bool need_flow) {
    need_hip(grad, "backwarp_backward");
    TORCH_CHECK(input.dim() == 4 && grad.sizes() == input.sizes() && flow.dim() == 4 && flow.size(1) == 2,
                "dbsr::backwarp_backward: grad / input [N,C,H,W], flow [N,2,H,W]");
    const int64_t N = input.size(0), C = input.size(1), H = input.size(2), W = input.size(3);
    const auto dt = input.scalar_type();
    at::Tensor din = at::empty({0}, input.options()), dfl = at::empty({0}, flow.options());
    if (!need_input && !need_flow) return {din, dfl};
    auto x = nhwc(input, r8(C), dt), g = nhwc(grad, r8(C), dt);
    auto fl = flow.permute({0, 2, 3, 1}).to(at::kFloat).contiguous();
    at::Tensor di32, df32;
    if (need_input) di32 = at::empty({N, H, W, r8(C)}, input.options().dtype(at::kFloat));
    if (need_flow) df32 = at::empty({N, H, W, 2}, input.options().dtype(at::kFloat));
    check(dbsr_backwarp_backward(N, H, W, C, desc(x, r8(C)), desc(fl, 2), 1.0f, desc(g, r8(C)),
                                 need_input ? desc(di32, r8(C)) : null_desc(), need_flow ? desc(df32, 2) : null_desc(),
                                 cur_stream()),
          "dbsr_backwarp_backward");
    if (need_input) din = nchw(di32, C).to(dt);
    if (need_flow) dfl = nchw(df32, 2).to(flow.scalar_type());
    return {din, dfl};
}

// feats [B,N,C,H,W] (frame 0 = the reference), logits [B,N,C,H,W] -> (fused [B,C,H,W], weights [B,N,C,H,W])
std::tuple<at::Tensor, at::Tensor> fuse_softmax(const at::Tensor& logits, const at::Tensor& feats, bool want_weights) {
    need_hip(logits, "fuse_softmax");
    TORCH_CHECK(logits.dim() == 5 && logits.sizes() == feats.sizes(), "dbsr::fuse_softmax: [B,N,C,H,W] inputs");
    const int64_t B = feats.size(0), N = feats.size(1), C = feats.size(2), H = feats.size(3), W = feats.size(4);
    TORCH_CHECK(C % 4 == 0, "dbsr::fuse_softmax: C % 4 == 0");
    const auto dt = feats.scalar_type();
    auto cl = [&](const at::Tensor& t) { return t.to(dt).reshape({B * N, C, H, W}).permute({0, 2, 3, 1}).contiguous(); };
    auto l = cl(logits), f = cl(feats);
    auto fused = at::empty({B, H, W, C}, feats.options());
    auto w = want_weights ? at::empty({B * N, H, W, C}, feats.options()) : at::Tensor();
    const int64_t img = H * W * C;
    check(dbsr_fuse_softmax(B, N, H * W, C, desc(l, C, 0, img), desc(f, C, 0, img, {1, (int)N, 0, 1}),
                            desc(f, C, 0, img, {(int)(N - 1), (int)N, 1, 1}), desc(fused, C, 0, img),
                            want_weights ? desc(w, C, 0, img) : null_desc(), cur_stream()),
          "dbsr_fuse_softmax");
    auto wout = want_weights ? w.view({B, N, H, W, C}).permute({0, 1, 4, 2, 3}).contiguous()
                             : at::empty({0}, feats.options());
    return {fused.permute({0, 3, 1, 2}).contiguous(), wout};
}

std::tuple<at::Tensor, at::Tensor> fuse_backward(const at::Tensor& weights, const at::Tensor& feats,
                                                 const at::Tensor& fused, const at::Tensor& dfused) {
    need_hip(weights, "fuse_backward");
    const int64_t B = feats.size(0), N = feats.size(1), C = feats.size(2), H = feats.size(3), W = feats.size(4);
    TORCH_CHECK(C % 8 == 0, "dbsr::fuse_backward: C % 8 == 0");
    const auto dt = feats.scalar_type();
    auto cl5 = [&](const at::Tensor& t) { return t.to(dt).reshape({-1, C, H, W}).permute({0, 2, 3, 1}).contiguous(); };
    auto w = cl5(weights), f = cl5(feats), fu = cl5(fused), dfu = cl5(dfused);
    auto dl = at::empty_like(w), df = at::empty_like(f);
    const int64_t img = H * W * C;
    check(dbsr_fuse_backward(B, N, H * W, C, desc(w, C, 0, img), desc(f, C, 0, img, {1, (int)N, 0, 1}),
                             desc(f, C, 0, img, {(int)(N - 1), (int)N, 1, 1}), desc(fu, C, 0, img),
                             desc(dfu, C, 0, img), desc(dl, C, 0, img), desc(df, C, 0, img, {1, (int)N, 0, 1}),
                             desc(df, C, 0, img, {(int)(N - 1), (int)N, 1, 1}), cur_stream()),
          "dbsr_fuse_backward");
    auto back = [&](const at::Tensor& t) { return t.view({B, N, H, W, C}).permute({0, 1, 4, 2, 3}).contiguous(); };
    return {back(dl), back(df)};
}

// Packed weights, one cache entry per weight tensor (repacking on every call is what made the op-level conv
// slow).  An entry is valid only while it describes the same live tensors: weak
// references to the weight's and the bias's TensorImpl (a freed tensor whose address a new one reuses never
// matches), their versions (an optimizer step bumps them and repacks once), data pointers, shapes and the
// compute dtype.  A stale entry is replaced, and entries of freed weights are evicted on every insert, so the
// cache holds at most one packed copy per live weight.  In-place writes that bypass version counting
// (`p.data.copy_(...)`, raw pointers) are invisible to it: call torch.ops.dbsr.clear_pack_cache() after them.
using WeakImpl = c10::weak_intrusive_ptr<c10::TensorImpl, c10::UndefinedTensorImpl>;
struct PackEntry {
    std::optional<WeakImpl> w, b;  // b empty when the conv has no bias
    int64_t w_version = -1, b_version = -1;
    const void* w_ptr = nullptr;
    const void* b_ptr = nullptr;
    std::vector<int64_t> w_shape;
    int dtype = -1;
    at::Tensor wp, bp;
};
std::mutex g_pack_mu;
std::map<const c10::TensorImpl*, PackEntry> g_pack_cache;

bool same_live(const std::optional<WeakImpl>& weak, const at::Tensor& t) {
    if (!weak) return false;
    auto strong = weak->lock();
    return strong.defined() && strong.get() == t.unsafeGetTensorImpl();
}

bool entry_valid(const PackEntry& e, const at::Tensor& w, const c10::optional<at::Tensor>& bias, int dc) {
    if (!same_live(e.w, w) || e.w_version != (int64_t)w._version() || e.w_ptr != w.data_ptr() ||
        e.w_shape != w.sizes().vec() || e.dtype != dc)
        return false;
    const bool has_b = bias.has_value() && bias->defined();
    if (has_b != e.bp.defined()) return false;
    if (has_b && (!same_live(e.b, *bias) || e.b_version != (int64_t)bias->_version() || e.b_ptr != bias->data_ptr()))
        return false;
    return true;
}

void clear_pack_cache() {
    std::lock_guard<std::mutex> lk(g_pack_mu);
    g_pack_cache.clear();
}

int64_t pack_cache_size() {
    std::lock_guard<std::mutex> lk(g_pack_mu);
    return (int64_t)g_pack_cache.size();
}

at::Tensor conv2d_fused(const at::Tensor& x, const at::Tensor& weight, const c10::optional<at::Tensor>& bias,
                        int64_t stride, int64_t padding, int64_t dilation, int64_t act,
                        const c10::optional<at::Tensor>& residual, int64_t post_act) {
    need_hip(x, "conv2d_fused");
    TORCH_CHECK(x.dim() == 4 && weight.dim() == 4 && weight.size(1) == x.size(1), "dbsr::conv2d_fused: shapes");
    const auto dt = x.scalar_type();
    const int dc = dcode(dt);
    const int64_t N = x.size(0), Cin = x.size(1), H = x.size(2), W = x.size(3);
    const int64_t Cout = weight.size(0), kh = weight.size(2), kw = weight.size(3);
    const int64_t oh = (H + 2 * padding - dilation * (kh - 1) - 1) / stride + 1;
    const int64_t ow = (W + 2 * padding - dilation * (kw - 1) - 1) / stride + 1;
    void* s = cur_stream();
    at::Tensor wp, bp;
    const bool has_b = bias.has_value() && bias->defined();
    if (has_b) TORCH_CHECK(bias->dim() == 1 && bias->size(0) == Cout, "dbsr::conv2d_fused: bias must be [Cout]");
    {
        std::lock_guard<std::mutex> lk(g_pack_mu);
        auto it = g_pack_cache.find(weight.unsafeGetTensorImpl());
        if (it != g_pack_cache.end() && entry_valid(it->second, weight, bias, dc)) {
            wp = it->second.wp;
            bp = it->second.bp;
        } else {
            auto w32 = weight.to(at::kFloat).contiguous();
            auto b32 = has_b ? bias->to(at::kFloat).contiguous() : at::Tensor();
            wp = at::empty({(int64_t)dbsr_conv_packed_elems(Cout, Cin, kh, kw)}, x.options());
            bp = has_b ? at::empty({Cout}, x.options().dtype(at::kFloat)) : at::Tensor();
            check(dbsr_conv_pack_weights(w32.data_ptr<float>(), has_b ? b32.data_ptr<float>() : nullptr,
                                         Cout, Cin, kh, kw, dc, 1, wp.data_ptr(),
                                         has_b ? bp.data_ptr<float>() : nullptr, s),
                  "dbsr_conv_pack_weights");
            // evict entries whose weight is gone, then (re)place this weight's entry
            for (auto e = g_pack_cache.begin(); e != g_pack_cache.end();)
                e = (!e->second.w || e->second.w->expired()) ? g_pack_cache.erase(e) : std::next(e);
            PackEntry ent;
            ent.w.emplace(weight.getIntrusivePtr());
            ent.w_version = weight._version();
            ent.w_ptr = weight.data_ptr();
            ent.w_shape = weight.sizes().vec();
            ent.dtype = dc;
            if (has_b) {
                ent.b.emplace(bias->getIntrusivePtr());
                ent.b_version = bias->_version();
                ent.b_ptr = bias->data_ptr();
            }
            ent.wp = wp;
            ent.bp = bp;
            g_pack_cache.insert_or_assign(weight.unsafeGetTensorImpl(), std::move(ent));
        }
    }
    auto xs = nhwc(x, conv_ld(Cin), dt);
    const int64_t ldy = r8(Cout);
    auto y = at::zeros({N, oh, ow, ldy}, x.options());
    at::Tensor rr;
    dbsr_conv_desc d{};
    d.n_frames = N;
    d.x = desc(xs, conv_ld(Cin));
    d.in_h = H; d.in_w = W; d.cin = Cin;
    d.w = wp.data_ptr();
    d.bias = has_b ? bp.data_ptr<float>() : nullptr;
    d.cout = Cout; d.kh = kh; d.kw = kw; d.stride = stride; d.pad = padding; d.dil = dilation;
    d.y = desc(y, ldy);
    d.out_h = oh; d.out_w = ow;
    d.act = act;
    if (residual.has_value()) {
        rr = nhwc(*residual, ldy, dt);
        d.res = desc(rr, ldy);
    } else {
        d.res = null_desc();
    }
    d.gate = null_desc();
    d.post_act = post_act;
    d.out_mode = DBSR_OUT_NHWC;
    d.shuffle = 0;
    const size_t need = dbsr_conv_workspace_bytes(&d);
    auto ws = at::zeros({(int64_t)std::max<size_t>(need / 4, 1)}, x.options().dtype(at::kFloat));
    d.workspace = ws.data_ptr();
    d.workspace_bytes = need;
    d.precise = 0;
    d.max_blocks = 0;
    check(dbsr_conv2d(&d, s), "dbsr_conv2d");
    return nchw(y, Cout);
}

// ------------------------------------------------------------------------------------------------
// PWC-Net training (csrc/pwc_grad.hip): the backward of conv2d_fused (act none / ReLU / LeakyReLU, no residual),
// ConvTranspose2d(k4, s2, p1) and the flow's final resize, forward and backward.
// ------------------------------------------------------------------------------------------------
at::Tensor f32_scratch(size_t bytes, const at::Tensor& like) {
    return at::empty({(int64_t)std::max<size_t>((bytes + 3) / 4, 4)}, like.options().dtype(at::kFloat));
}

// a plain dbsr_conv2d of NHWC `xs` (ld = conv_ld(cin)) with torch-layout fp32 weights, no bias / activation
at::Tensor run_conv(const at::Tensor& xs, int64_t N, int64_t H, int64_t W, int64_t cin, const at::Tensor& w32,
                    int64_t cout, int64_t k, int64_t stride, int64_t pad, int64_t dil, int64_t oh, int64_t ow) {
    void* s = cur_stream();
    auto wp = at::empty({(int64_t)dbsr_conv_packed_elems(cout, cin, k, k)}, xs.options());
    check(dbsr_conv_pack_weights(w32.data_ptr<float>(), nullptr, cout, cin, k, k, dcode(xs.scalar_type()), 1,
                                 wp.data_ptr(), nullptr, s),
          "dbsr_conv_pack_weights");
    auto y = at::zeros({N, oh, ow, r8(cout)}, xs.options());
    dbsr_conv_desc d{};
    d.n_frames = N;
    d.x = desc(xs, conv_ld(cin));
    d.in_h = H; d.in_w = W; d.cin = cin;
    d.w = wp.data_ptr();
    d.bias = nullptr;
    d.cout = cout; d.kh = k; d.kw = k; d.stride = stride; d.pad = pad; d.dil = dil;
    d.y = desc(y, r8(cout));
    d.out_h = oh; d.out_w = ow;
    d.act = DBSR_ACT_NONE;
    d.res = null_desc();
    d.gate = null_desc();
    d.out_mode = DBSR_OUT_NHWC;
    const size_t need = dbsr_conv_workspace_bytes(&d);
    auto ws = at::zeros({(int64_t)std::max<size_t>(need / 4, 1)}, xs.options().dtype(at::kFloat));
    d.workspace = ws.data_ptr();
    d.workspace_bytes = need;
    check(dbsr_conv2d(&d, s), "dbsr_conv2d");
    return y;
}

at::Tensor chan_sum(const at::Tensor& t, int64_t N, int64_t hw, int64_t C, int64_t ld) {
    auto out = at::empty({C}, t.options().dtype(at::kFloat));
    const size_t need = dbsr_chan_sum_workspace_bytes(N, hw, C);
    auto ws = f32_scratch(need, t);
    check(dbsr_chan_sum(N, hw, C, desc(t, ld), out.data_ptr<float>(), 0, ws.data_ptr(), need, cur_stream()),
          "dbsr_chan_sum");
    return out;
}

// (an unwanted gradient is returned as an empty tensor and is not computed)
std::tuple<at::Tensor, at::Tensor, at::Tensor> conv2d_backward(const at::Tensor& grad, const at::Tensor& x,
                                                               const at::Tensor& weight, const at::Tensor& out,
                                                               int64_t stride, int64_t padding, int64_t dilation,
                                                               int64_t act, bool need_x, bool need_w, bool need_b) {
    need_hip(grad, "conv2d_backward");
    need_hip(x, "conv2d_backward");
    need_hip(weight, "conv2d_backward");
    TORCH_CHECK(x.dim() == 4 && weight.dim() == 4 && grad.dim() == 4 && weight.size(1) == x.size(1) &&
                weight.size(2) == weight.size(3) && grad.size(0) == x.size(0) && grad.size(1) == weight.size(0),
                "dbsr::conv2d_backward: shapes");
    TORCH_CHECK(act == DBSR_ACT_NONE || act == DBSR_ACT_RELU || act == DBSR_ACT_LRELU, "dbsr::conv2d_backward: act");
    const auto dt = x.scalar_type();
    const int dc = dcode(dt);
    const int64_t N = x.size(0), Cin = x.size(1), H = x.size(2), W = x.size(3);
    const int64_t Cout = weight.size(0), k = weight.size(2), oh = grad.size(2), ow = grad.size(3);
    at::Tensor dx = at::empty({0}, x.options()), dw = at::empty({0}, weight.options()),
               db = at::empty({0}, weight.options());
    if (!need_x && !need_w && !need_b) return {dx, dw, db};
    void* s = cur_stream();
    const int64_t ldc = conv_ld(Cout);
    auto dpre = nhwc(grad, ldc, dt);
    if (act != DBSR_ACT_NONE) {
        need_hip(out, "conv2d_backward");
        TORCH_CHECK(out.sizes() == grad.sizes(), "dbsr::conv2d_backward: out must be the forward's output");
        auto o = nhwc(out, ldc, dt), g = dpre;
        dpre = at::zeros_like(g);
        check(dbsr_act_backward(N, oh * ow, Cout, act, desc(g, ldc), desc(o, ldc), desc(dpre, ldc), s),
              "dbsr_act_backward");
    }
    if (need_w) {
        auto xs = nhwc(x, r8(Cin), dt);
        auto dw32 = at::empty({Cout, Cin, k, k}, x.options().dtype(at::kFloat));
        at::Tensor db32;
        if (need_b) db32 = at::empty({Cout}, x.options().dtype(at::kFloat));
        float* dbp = need_b ? db32.data_ptr<float>() : nullptr;
        if ((k == 1 || k == 3) && stride == 1 && dilation == 1 && padding == k / 2) {
            const size_t need = dbsr_conv_wgrad_workspace_bytes(N, H, W, Cin, Cout, k);
            auto ws = f32_scratch(need, x);
            check(dbsr_conv_wgrad_bias(N, H, W, desc(xs, r8(Cin)), Cin, desc(dpre, ldc), Cout, k, dw32.data_ptr<float>(),
                                       dbp, 0, ws.data_ptr(), need, s),
                  "dbsr_conv_wgrad_bias");
        } else {
            const size_t need = dbsr_conv_wgrad_sd_workspace_bytes(N, oh, ow, Cin, Cout, k);
            auto ws = f32_scratch(need, x);
            check(dbsr_conv_wgrad_sd(N, H, W, desc(xs, r8(Cin)), Cin, oh, ow, desc(dpre, ldc), Cout, k, stride, dilation,
                                     padding, dw32.data_ptr<float>(), dbp, 0, ws.data_ptr(), need, s),
                  "dbsr_conv_wgrad_sd");
        }
        dw = dw32.to(weight.scalar_type());
        if (need_b) db = db32.to(weight.scalar_type());
    } else if (need_b) {
        db = chan_sum(dpre, N, oh * ow, Cout, ldc).to(weight.scalar_type());
    }
    if (need_x) {
        auto w32 = weight.to(at::kFloat).contiguous();
        const int64_t padt = dilation * (k - 1) - padding;
        if (stride == 1 && padt >= 0) {
            // the stride-1 route: the forward conv over dpre with dbsr_dgrad_weights
            auto wt = at::empty({Cin, Cout, k, k}, w32.options());
            check(dbsr_dgrad_weights(w32.data_ptr<float>(), Cout, Cin, k, k, wt.data_ptr<float>(), s),
                  "dbsr_dgrad_weights");
            dx = nchw(run_conv(dpre, N, oh, ow, Cout, wt, Cin, k, 1, padt, dilation, H, W), Cin);
        } else {
            auto wp = at::empty({(int64_t)dbsr_dgrad_sd_packed_elems(Cout, Cin, k)}, x.options());
            check(dbsr_dgrad_sd_pack(w32.data_ptr<float>(), Cout, Cin, k, dc, wp.data_ptr(), s), "dbsr_dgrad_sd_pack");
            auto y = at::empty({N, H, W, r8(Cin)}, x.options());
            check(dbsr_conv_dgrad_sd(N, H, W, desc(y, r8(Cin)), Cin, oh, ow, desc(dpre, ldc), Cout, k, stride, dilation,
                                     padding, wp.data_ptr(), s),
                  "dbsr_conv_dgrad_sd");
            dx = nchw(y, Cin);
        }
    }
    return {dx, dw, db};
}

// nn.ConvTranspose2d(cin -> cout <= 4, k 4, s 2, p 1): weight torch's [cin][cout][4][4]
at::Tensor conv_transpose2d_k4s2(const at::Tensor& x, const at::Tensor& weight, const c10::optional<at::Tensor>& bias) {
    need_hip(x, "conv_transpose2d_k4s2");
    need_hip(weight, "conv_transpose2d_k4s2");
    TORCH_CHECK(x.dim() == 4 && weight.dim() == 4 && weight.size(0) == x.size(1) && weight.size(2) == 4 &&
                weight.size(3) == 4 && weight.size(1) >= 1 && weight.size(1) <= 4,
                "dbsr::conv_transpose2d_k4s2: x [N,Cin,H,W], weight [Cin,Cout<=4,4,4]");
    const auto dt = x.scalar_type();
    const int64_t N = x.size(0), Cin = x.size(1), H = x.size(2), W = x.size(3), Cout = weight.size(1);
    const bool has_b = bias.has_value() && bias->defined();
    if (has_b) {
        need_hip(*bias, "conv_transpose2d_k4s2");
        TORCH_CHECK(bias->dim() == 1 && bias->size(0) == Cout, "dbsr::conv_transpose2d_k4s2: bias must be [Cout]");
    }
    auto xs = nhwc(x, r8(Cin), dt);
    // [ky][kx][cout][cin8] fp32, channels zero-padded
    auto wr = at::zeros({4, 4, Cout, r8(Cin)}, x.options().dtype(at::kFloat));
    wr.narrow(3, 0, Cin).copy_(weight.to(at::kFloat).permute({2, 3, 1, 0}));
    auto b32 = has_b ? bias->to(at::kFloat).contiguous() : at::zeros({Cout}, x.options().dtype(at::kFloat));
    auto out = at::empty({N, 2 * H, 2 * W, Cout}, x.options().dtype(at::kFloat));
    check(dbsr_conv_transpose_k4s2(N, H, W, Cin, Cout, desc(xs, r8(Cin)), wr.data_ptr<float>(), b32.data_ptr<float>(),
                                   desc(out, Cout), cur_stream()),
          "dbsr_conv_transpose_k4s2");
    return out.permute({0, 3, 1, 2}).contiguous().to(dt);
}

std::tuple<at::Tensor, at::Tensor, at::Tensor> conv_transpose2d_k4s2_backward(const at::Tensor& grad, const at::Tensor& x,
                                                                              const at::Tensor& weight, bool need_x,
                                                                              bool need_w, bool need_b) {
    need_hip(grad, "conv_transpose2d_k4s2_backward");
    need_hip(x, "conv_transpose2d_k4s2_backward");
    need_hip(weight, "conv_transpose2d_k4s2_backward");
    TORCH_CHECK(x.dim() == 4 && weight.dim() == 4 && grad.dim() == 4 && weight.size(0) == x.size(1) &&
                weight.size(2) == 4 && weight.size(3) == 4 && grad.size(1) == weight.size(1) &&
                grad.size(2) == 2 * x.size(2) && grad.size(3) == 2 * x.size(3),
                "dbsr::conv_transpose2d_k4s2_backward: shapes");
    const auto dt = x.scalar_type();
    const int64_t N = x.size(0), Cin = x.size(1), H = x.size(2), W = x.size(3), Cout = weight.size(1);
    at::Tensor dx = at::empty({0}, x.options()), dw = at::empty({0}, weight.options()),
               db = at::empty({0}, weight.options());
    if (!need_x && !need_w && !need_b) return {dx, dw, db};
    void* s = cur_stream();
    const int64_t ldg = conv_ld(Cout);
    auto g = nhwc(grad, ldg, dt);
    if (need_x) {
        // a k4 s2 p1 conv over dy whose weights are the transposed conv's as they are: [Cin][Cout][4][4]
        auto w32 = weight.to(at::kFloat).contiguous();
        dx = nchw(run_conv(g, N, 2 * H, 2 * W, Cout, w32, Cin, 4, 2, 1, 1, H, W), Cin);
    }
    if (need_w) {
        // the roles swapped: "input" = dy (2H x 2W, Cout channels), "output gradient" = x (H x W, Cin channels)
        auto xs = nhwc(x, r8(Cin), dt);
        auto dw32 = at::empty({Cin, Cout, 4, 4}, x.options().dtype(at::kFloat));
        const size_t need = dbsr_conv_wgrad_sd_workspace_bytes(N, H, W, Cout, Cin, 4);
        auto ws = f32_scratch(need, x);
        check(dbsr_conv_wgrad_sd(N, 2 * H, 2 * W, desc(g, ldg), Cout, H, W, desc(xs, r8(Cin)), Cin, 4, 2, 1, 1,
                                 dw32.data_ptr<float>(), nullptr, 0, ws.data_ptr(), need, s),
              "dbsr_conv_wgrad_sd");
        dw = dw32.to(weight.scalar_type());
    }
    if (need_b) db = chan_sum(g, N, 4 * H * W, Cout, ldg).to(weight.scalar_type());
    return {dx, dw, db};
}

// pwcnet.py:274-279: 20 * bilinear(flow -> H x W) * (W / Wp, H / Hp); Hp / Wp 0: four times the flow's size
at::Tensor flow_finalize(const at::Tensor& flow, int64_t H, int64_t W, int64_t Hp, int64_t Wp) {
    need_hip(flow, "flow_finalize");
    TORCH_CHECK(flow.dim() == 4 && flow.size(1) == 2 && H > 0 && W > 0, "dbsr::flow_finalize: flow [P,2,hf,wf], H, W > 0");
    const int64_t P = flow.size(0), hf = flow.size(2), wf = flow.size(3);
    if (Hp <= 0) Hp = 4 * hf;
    if (Wp <= 0) Wp = 4 * wf;
    auto fl = flow.permute({0, 2, 3, 1}).to(at::kFloat).contiguous();
    auto out = at::empty({P, 2, H, W}, flow.options().dtype(at::kFloat));
    check(dbsr_flow_finalize(P, 2, hf, wf, desc(fl, 2), H, W, Hp, Wp, out.data_ptr<float>(), 0.0f, null_desc(),
                             cur_stream()),
          "dbsr_flow_finalize");
    return out.to(flow.scalar_type());
}

at::Tensor flow_finalize_backward(const at::Tensor& grad, int64_t hf, int64_t wf, int64_t Hp, int64_t Wp) {
    need_hip(grad, "flow_finalize_backward");
    TORCH_CHECK(grad.dim() == 4 && grad.size(1) == 2 && hf > 0 && wf > 0, "dbsr::flow_finalize_backward: grad [P,2,H,W]");
    const int64_t P = grad.size(0), H = grad.size(2), W = grad.size(3);
    if (Hp <= 0) Hp = 4 * hf;
    if (Wp <= 0) Wp = 4 * wf;
    auto g = grad.to(at::kFloat).contiguous();
    auto out = at::empty({P, hf, wf, 2}, grad.options().dtype(at::kFloat));
    check(dbsr_flow_finalize_backward(P, hf, wf, H, W, Hp, Wp, g.data_ptr<float>(), desc(out, 2), cur_stream()),
          "dbsr_flow_finalize_backward");
    return out.permute({0, 3, 1, 2}).contiguous().to(grad.scalar_type());
}

// F.interpolate(x, (Hp, Wp), mode='bilinear', align_corners=False), forward only (pwcnet.py:266-271: the images)
at::Tensor resize_bilinear(const at::Tensor& x, int64_t Hp, int64_t Wp) {
    need_hip(x, "resize_bilinear");
    TORCH_CHECK(x.dim() == 4 && Hp > 0 && Wp > 0, "dbsr::resize_bilinear: x [N,C,H,W], Hp, Wp > 0");
    const int64_t N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
    auto in = x.to(at::kFloat).contiguous();
    auto out = at::empty({N, C, Hp, Wp}, x.options().dtype(at::kFloat));
    check(dbsr_resize_bilinear(N * C, H, W, in.data_ptr<float>(), Hp, Wp, (float)H / (float)Hp, (float)W / (float)Wp,
                               1.0f, out.data_ptr<float>(), cur_stream()),
          "dbsr_resize_bilinear");
    return out.to(x.scalar_type());
}

}  // namespace

TORCH_LIBRARY(dbsr, m) {
    m.def("conv2d_backward(Tensor grad, Tensor x, Tensor weight, Tensor out, int stride, int padding, int dilation, "
          "int act, bool need_x, bool need_w, bool need_b) -> (Tensor, Tensor, Tensor)");
    m.def("conv_transpose2d_k4s2(Tensor x, Tensor weight, Tensor? bias=None) -> Tensor");
    m.def("conv_transpose2d_k4s2_backward(Tensor grad, Tensor x, Tensor weight, bool need_x, bool need_w, bool need_b) "
          "-> (Tensor, Tensor, Tensor)");
    m.def("flow_finalize(Tensor flow, int H, int W, int Hp=0, int Wp=0) -> Tensor");
    m.def("flow_finalize_backward(Tensor grad, int hf, int wf, int Hp=0, int Wp=0) -> Tensor");
    m.def("resize_bilinear(Tensor x, int Hp, int Wp) -> Tensor");
    m.def("correlation(Tensor first, Tensor second, bool leaky=False) -> Tensor");
    m.def("correlation_backward(Tensor grad, Tensor first, Tensor second, Tensor out, bool leaky) -> (Tensor, Tensor)");
    m.def("backwarp(Tensor input, Tensor flow) -> Tensor");
    m.def("warp_bilinear(Tensor feat, Tensor flow) -> Tensor");
    m.def("warp_bilinear_backward(Tensor grad, Tensor flow) -> Tensor");
    m.def("warp_bilinear_flow_backward(Tensor grad, Tensor feat, Tensor flow) -> Tensor");
    m.def("backwarp_backward(Tensor grad, Tensor input, Tensor flow, bool need_input=True, bool need_flow=True) -> "
          "(Tensor, Tensor)");
    m.def("fuse_softmax(Tensor logits, Tensor feats, bool want_weights=True) -> (Tensor, Tensor)");
    m.def("fuse_backward(Tensor weights, Tensor feats, Tensor fused, Tensor dfused) -> (Tensor, Tensor)");
    m.def("conv2d_fused(Tensor x, Tensor weight, Tensor? bias=None, int stride=1, int padding=0, int dilation=1, "
          "int act=0, Tensor? residual=None, int post_act=0) -> Tensor");
    m.def("clear_pack_cache() -> ()");
    m.impl("clear_pack_cache", &clear_pack_cache);
    m.def("pack_cache_size() -> int");
    m.impl("pack_cache_size", &pack_cache_size);
}

// the ROCm build of PyTorch dispatches HIP tensors under the CUDA key
TORCH_LIBRARY_IMPL(dbsr, CUDA, m) {
    m.impl("correlation", &correlation);
    m.impl("correlation_backward", &correlation_backward);
    m.impl("backwarp", &backwarp);
    m.impl("warp_bilinear", &warp_bilinear);
    m.impl("warp_bilinear_backward", &warp_bilinear_backward);
    m.impl("warp_bilinear_flow_backward", &warp_bilinear_flow_backward);
    m.impl("backwarp_backward", &backwarp_backward);
    m.impl("fuse_softmax", &fuse_softmax);
    m.impl("fuse_backward", &fuse_backward);
    m.impl("conv2d_fused", &conv2d_fused);
    m.impl("conv2d_backward", &conv2d_backward);
    m.impl("conv_transpose2d_k4s2", &conv_transpose2d_k4s2);
    m.impl("conv_transpose2d_k4s2_backward", &conv_transpose2d_k4s2_backward);
    m.impl("flow_finalize", &flow_finalize);
    m.impl("flow_finalize_backward", &flow_finalize_backward);
    m.impl("resize_bilinear", &resize_bilinear);
}
