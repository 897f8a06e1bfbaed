// Host runtime of the network path: the handle (ph_model_create / ph_model_destroy), weight re-packing, the options table and the small accessors of the
// C ABI (ph_model_*); the workspace plan is plan.hip, the forward launch sequence forward.hip.  Together they replace TorchBackend.__call__ ->
// LightningModule.forward -> Model.forward -> UNet.forward of the reference
// (sleap_nn/inference/layers/backends/torch_backend.py:113-153,
//  training/lightning_modules.py:1840-1848, architectures/model.py:237-261,
//  architectures/unet.py:260-299).
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <mutex>
#include <type_traits>
#include <vector>

#include "model_internal.h"
#include "train_kernels.h"

namespace ph {

static thread_local std::string g_err;

void set_error(const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
}

}  // namespace ph

namespace ph {

int device_cu_count(int* out) {
  static std::atomic<int> cache[64];  // zero-initialised; a count is a device property, racing writers store the same value
  int dev = 0;
  PH_HIP_CHECK(hipGetDevice(&dev));
  int n = (dev >= 0 && dev < 64) ? cache[dev].load(std::memory_order_relaxed) : 0;
  if (!n) {
    PH_HIP_CHECK(hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev));
    if (dev >= 0 && dev < 64) cache[dev].store(n, std::memory_order_relaxed);
  }
  *out = n;
  return PH_OK;
}

int upload(ph_model* m, const std::vector<float>& host, float** dev) {
  void* p = nullptr;
  PH_HIP_CHECK(hipMalloc(&p, std::max<size_t>(host.size(), 4) * sizeof(float)));
  m->allocs.push_back(p);
  PH_HIP_CHECK(hipMemcpy(p, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice));
  *dev = static_cast<float*>(p);
  return PH_OK;
}

int upload_ints(ph_model* m, const std::vector<int>& host, int** dev) {
  void* p = nullptr;
  PH_HIP_CHECK(hipMalloc(&p, std::max<size_t>(host.size(), 4) * sizeof(int)));
  m->allocs.push_back(p);
  PH_HIP_CHECK(hipMemcpy(p, host.data(), host.size() * sizeof(int), hipMemcpyHostToDevice));
  *dev = static_cast<int*>(p);
  return PH_OK;
}

// Upload a packed value array together with its gather map.  `packed_idx` is the SAME packing
// applied to an array holding (canonical index + 1) as doubles (exact for any arena size).
static int upload_packed(ph_model* m, const std::vector<float>& packed_val, const std::vector<double>& packed_idx, float** dev) {
  int rc = upload(m, packed_val, dev);
  if (rc != PH_OK) return rc;
  std::vector<int> map(packed_idx.size());
  for (size_t i = 0; i < packed_idx.size(); ++i) map[i] = (int)((int64_t)packed_idx[i] - 1);
  PackedBuffer pb;
  pb.dst = *dev;
  pb.n = packed_val.size();
  rc = upload_ints(m, map, &pb.map);
  if (rc != PH_OK) return rc;
  m->packed.push_back(pb);
  return PH_OK;
}

// Note a buffer that is computed on the device from `src`, so that ph_model_set_params recomputes it
static DerivedBuffer& add_derived(ph_model* m, DerivedKind kind, const float* src, float* dst, int panels = 0, int bn = 0) {
  DerivedBuffer db;
  db.kind = kind;
  db.src = src;
  db.dst = dst;
  db.panels = panels;
  db.bn = bn;
  m->derived.push_back(db);
  return m->derived.back();
}

// Run one packing routine twice -- on the weight values and on their canonical indices -- and upload both.
template <typename PackFn>
static int pack_upload(ph_model* m, PackFn&& pack, const float* values, const std::vector<double>& indices, float** dev) {
  std::vector<float> v;
  std::vector<double> x;
  pack(values, v);
  pack(indices.data(), x);
  return upload_packed(m, v, x, dev);
}

// OIHW (cout, cin_total, 3, 3) -> the conv weight of the data gradient wrt channels
// [ci_off, ci_off + cin_part): Wd[o = ci][i = co][ky][kx] = W[co][ci_off + ci][2-ky][2-kx].
template <typename T>
static void dgrad_weight(const T* w, int cout, int cin_total, int ci_off, int cin_part, std::vector<T>& out, int k = 3) {
  out.assign((size_t)cin_part * cout * k * k, T(0));
  for (int ci = 0; ci < cin_part; ++ci)
    for (int co = 0; co < cout; ++co)
      for (int ky = 0; ky < k; ++ky)
        for (int kx = 0; kx < k; ++kx)
          out[(((size_t)ci * cout + co) * k + ky) * k + kx] = w[(((size_t)co * cin_total + ci_off + ci) * k + (k - 1 - ky)) * k + (k - 1 - kx)];
}

// Conv2d OIHW (cout, cin0+cin1, 3, 3) or ConvTranspose2d IOHW (cin0, cout, 3, 3) ->
// [n_tile][chunk][tap][bn][16] with channel/row padding zeros.
template <typename T>
static void pack_conv(const T* w, bool transposed, int cin0, int cin1, int cout, int bn, std::vector<T>& out) {
  const int c0p = pad16(cin0), c1p = cin1 > 0 ? pad16(cin1) : 0;
  const int coutp = pad16(cout);
  const int ntiles = (coutp + bn - 1) / bn;
  const int ch0 = c0p / 16, ch1 = c1p / 16, nch = ch0 + ch1;
  const int cin = cin0 + cin1;
  out.assign((size_t)ntiles * nch * 9 * bn * 16, T(0));
  for (int nt = 0; nt < ntiles; ++nt)
    for (int ch = 0; ch < nch; ++ch)
      for (int tap = 0; tap < 9; ++tap) {
        const int ky = tap / 3, kx = tap % 3;
        for (int n = 0; n < bn; ++n) {
          const int co = nt * bn + n;
          if (co >= cout) continue;
          for (int kc = 0; kc < 16; ++kc) {
            int ci;
            if (ch < ch0) {
              const int c = ch * 16 + kc;
              if (c >= cin0) continue;
              ci = c;
            } else {
              const int c = (ch - ch0) * 16 + kc;
              if (c >= cin1) continue;
              ci = cin0 + c;
            }
            T v;
            if (!transposed)
              v = w[(((size_t)co * cin + ci) * 3 + ky) * 3 + kx];
            else  // flipped, in/out swapped: Wc[co][ci][ky][kx] = Wt[ci][co][2-ky][2-kx]
              v = w[(((size_t)ci * cout + co) * 3 + (2 - ky)) * 3 + (2 - kx)];
            out[((((size_t)nt * nch + ch) * 9 + tap) * bn + n) * 16 + kc] = v;
          }
        }
      }
}

// [n_tile][chunk][tap][bn][16] -> [n_tile][chunk][piece = (tap*bn + n)/16][quad q][row r = (tap*bn+n)%16][4]
// (the order in which one LDS-DMA wave-instruction writes a 1-KiB piece, see conv3x3_mfma_dma_kernel)
// [tap][ci 16][co 16] (zero padded) from OIHW, for conv3x3_c16_kernel
template <typename T>
static void pack_c16(const T* w, int cout, int cin, std::vector<T>& out) {
  out.assign(9 * 256, T(0));
  for (int co = 0; co < cout; ++co)
    for (int ci = 0; ci < cin; ++ci)
      for (int tap = 0; tap < 9; ++tap) out[(size_t)(tap * 16 + ci) * 16 + co] = w[((size_t)co * cin + ci) * 9 + tap];
}

template <typename T>
static void repack_dma(const std::vector<T>& in, int bn, std::vector<T>& out) {
  out.resize(in.size());
  const size_t panel = (size_t)9 * bn * 16;
  for (size_t base = 0; base < in.size(); base += panel)
    for (int row = 0; row < 9 * bn; ++row)
      for (int k = 0; k < 16; ++k) {
        const int piece = row >> 4, r = row & 15, q = k >> 2, e = k & 3;
        out[base + (size_t)piece * 256 + q * 64 + r * 4 + e] = in[base + (size_t)row * 16 + k];
      }
}

// Row-GEMM weights (gemm_mfma_dma_kernel): Linear (cout, cin) [taps = 1], Conv2d k2 s2 (cout, cin, 2, 2)
// [taps = 4] or Conv2d 3x3 over concat(cin0, cin1) (cout, cin0 + cin1, 3, 3) [taps = 9] ->
// [n_tile][stage][piece = n / 8][slot][row n % 8][4]; a stage is 32 channels of one source at one tap,
// stage order = source, 32-channel slice, tap (taps innermost); slot = channel quad ^ (piece & 1)
// (the LDS image the kernel's DMA writes); zero-padded channels / rows.
// CNBlock MLP, first Linear (4C, C) -> [hidden block hb][piece q: C / 8][lane (i = lane & 31, h = lane >> 5)][t]: W1[hb 32 + i][h C / 2 + 4 q + t]
// (the A operand of K step s = 4 q + t of cnblock_mlp_kernel's first product: channels (s, C / 2 + s) in the two lane halves)
template <typename T>
static void pack_mlp_w1(const T* w, int c, std::vector<T>& out) {
  const int nhb = 4 * c / 32, p1 = c / 8;
  out.assign((size_t)nhb * p1 * 256, T(0));
  for (int hb = 0; hb < nhb; ++hb)
    for (int q = 0; q < p1; ++q)
      for (int lane = 0; lane < 64; ++lane)
        for (int t = 0; t < 4; ++t) out[(((size_t)hb * p1 + q) * 64 + lane) * 4 + t] = w[(size_t)(hb * 32 + (lane & 31)) * c + (lane >> 5) * (c / 2) + 4 * q + t];
}
// ... second Linear (C, 4C) -> [hb][piece nb 4 + g][lane (n = lane & 31, h)][t]: W2[nb 32 + n][hb 32 + 8 g + 4 h + t]: K step r = 4 g + t of the chained product is
// the pair of hidden channels that accumulator register r of the first product holds in the two lane halves
template <typename T>
static void pack_mlp_w2(const T* w, int c, std::vector<T>& out) {
  const int nhb = 4 * c / 32, nb_ = c / 32;
  out.assign((size_t)nhb * nb_ * 4 * 256, T(0));
  for (int hb = 0; hb < nhb; ++hb)
    for (int nb = 0; nb < nb_; ++nb)
      for (int g = 0; g < 4; ++g)
        for (int lane = 0; lane < 64; ++lane)
          for (int t = 0; t < 4; ++t)
            out[((((size_t)hb * nb_ + nb) * 4 + g) * 64 + lane) * 4 + t] = w[(size_t)(nb * 32 + (lane & 31)) * (4 * c) + hb * 32 + 8 * g + 4 * (lane >> 5) + t];
}

template <typename T>
static void pack_gemm(const T* w, int cout, int cin0, int cin1, int taps, int bn, std::vector<T>& out) {
  const int c0p = pad16(cin0), c1p = cin1 > 0 ? pad16(cin1) : 0, coutp = pad16(cout);
  const int ntiles = (coutp + bn - 1) / bn;
  const int sl0 = (c0p + 31) / 32, sl1 = (c1p + 31) / 32;
  const int total = (sl0 + sl1) * taps, bp = bn / 8, cin = cin0 + cin1;
  out.assign((size_t)ntiles * total * bp * 256, T(0));
  for (int nt = 0; nt < ntiles; ++nt)
    for (int st = 0; st < total; ++st) {
      const int slice = st / taps, tap = st % taps;
      const bool second = slice >= sl0;
      const int c0 = (second ? slice - sl0 : slice) * 32;
      for (int pb = 0; pb < bp; ++pb)
        for (int slot = 0; slot < 8; ++slot)
          for (int r = 0; r < 8; ++r)
            for (int e = 0; e < 4; ++e) {
              const int co = nt * bn + pb * 8 + r, c = c0 + (slot ^ (pb & 1)) * 4 + e;
              if (co >= cout || c >= (second ? cin1 : cin0)) continue;
              const int ci = second ? cin0 + c : c;
              out[(((size_t)nt * total + st) * bp + pb) * 256 + slot * 32 + r * 4 + e] = w[((size_t)co * cin + ci) * taps + tap];
            }
    }
}

int choose_bn(int coutp) { return coutp >= 64 ? 64 : 32; }

void apply_conv_options(const ph_model* m, ConvArgs& a) {
  a.use_wino = m->conv_wino;
  a.use_wino2d = m->conv_wino2d;
  a.wino4_min_cin = m->conv_wino4_min_cin;
  a.use_w16 = m->conv_w16;
  a.persist = m->conv_persist;
  a.use_c16 = m->conv_c16;
  a.dma_stagger = m->dma_stagger;
  a.splitk = m->conv_splitk;  // (ph_model_forward clears it for a training plan unless a slice count is forced)
  a.split_counters = m->split_counters_dev;
  a.split_counters_n = m->split_counters_dev ? 4096 : 0;  // (units; the buffer holds three words per unit)
  a.splitk_finish = m->conv_splitk_finish;
  a.use_sm = 0;  // (ph_model_forward: the kind of plan decides)
}

// fp16 weight packs of every 3x3 conv / transposed conv, derived on the device from the fp32 LDS-DMA panels the first time a
// forward needs them (and again after every ph_model_set_params, through m->derived).  Allocates: not capturable -- a
// hipGraph user runs one eager forward first (HipBackend does).
int ensure_f16_weights(ph_model* m, int plain, hipStream_t s) {
  for (PackedOp& op : m->ops) {
    const ph_op_desc& d = op.d;
    if ((d.kind != PH_OP_CONV && d.kind != PH_OP_CONVT) || op.w_f16_dev[plain]) continue;
    PH_REQUIRE(op.w_dma_dev && (op.bn == 32 || op.bn == 64), "conv op has no LDS-DMA weight panels");
    const int chunks0 = pad16(d.cin0) / 16, chunks1 = d.cin1 > 0 ? pad16(d.cin1) / 16 : 0;
    const int n_tiles = (pad16(d.cout) + op.bn - 1) / op.bn;
    float* w = nullptr;
    PH_HIP_CHECK(hipMalloc(&w, (size_t)f16_weight_pack_floats(n_tiles, chunks0, chunks1, op.bn, plain) * sizeof(float)));
    m->allocs.push_back(w);
    int rc = launch_f16_weight_pack(op.w_dma_dev, w, n_tiles, chunks0, chunks1, op.bn, plain, s);
    if (rc != PH_OK) return rc;
    DerivedBuffer& db = add_derived(m, DERIVED_F16_PACK, op.w_dma_dev, w, 0, op.bn);
    db.n_tiles = n_tiles;
    db.chunks0 = chunks0;
    db.chunks1 = chunks1;
    db.plain = plain;
    op.w_f16_dev[plain] = w;
  }
  return PH_OK;
}

int drain_events(ph_model* m) {
  if (!m->events_pending) return PH_OK;
  const size_t n = m->ops.size();
  PH_HIP_CHECK(hipEventSynchronize(m->ev[n]));
  for (size_t i = 0; i < n; ++i) {
    float ms = 0.f;
    PH_HIP_CHECK(hipEventElapsedTime(&ms, m->ev[i], m->ev[i + 1]));
    m->op_ms[i] += ms;
  }
  m->profiled_forwards += 1;
  m->events_pending = false;
  return PH_OK;
}

}  // namespace ph

using namespace ph;

extern "C" {

const char* ph_last_error(void) { return ph::g_err.c_str(); }
int ph_version(void) { return PH_VERSION; }

ph_model* ph_model_create(const ph_op_desc* ops, int32_t n_ops, const float* const* weights, const int64_t* weight_numel,
                          int32_t n_weights, int32_t n_slots, int32_t n_outputs) {
  if (!ops || n_ops <= 0 || n_slots <= 0) {
    set_error("ph_model_create: empty program");
    return nullptr;
  }
  if (prepare_kernels() != PH_OK || prepare_convnext_kernels() != PH_OK || prepare_f16_kernels() != PH_OK) return nullptr;
  ph_model* m = new ph_model();
  m->n_slots = n_slots;
  m->n_outputs = n_outputs;
  {
    std::vector<float> z(64, 0.f);
    if (upload(m, z, &m->zeros_dev) != PH_OK) {
      ph_model_destroy(m);
      return nullptr;
    }
    std::vector<float> zc(3 * 4096, 0.f);  // (uploaded as floats: all-zero bits either way; arrivals | claimed shares | departures per split-K unit)
    float* cdev = nullptr;
    if (upload(m, zc, &cdev) != PH_OK) {
      ph_model_destroy(m);
      return nullptr;
    }
    m->split_counters_dev = reinterpret_cast<unsigned*>(cdev);
  }
  auto fail = [&](const char* msg, int i) -> ph_model* {
    set_error("ph_model_create: op %d: %s", i, msg);
    ph_model_destroy(m);
    return nullptr;
  };
  // canonical parameter arena = weights[] concatenated in the given order
  m->weight_offset.resize(n_weights);
  m->weight_numel.assign(weight_numel, weight_numel + n_weights);
  for (int i = 0; i < n_weights; ++i) {
    m->weight_offset[i] = m->n_params;
    m->n_params += weight_numel[i];
  }
  if (m->n_params >= (int64_t)1 << 31) return (set_error("models with >= 2^31 parameters are not supported"), ph_model_destroy(m), nullptr);
  auto index_array = [&](int wi) {
    std::vector<double> v((size_t)(wi >= 0 ? weight_numel[wi] : 0));
    for (size_t k = 0; k < v.size(); ++k) v[k] = (double)(m->weight_offset[wi] + (int64_t)k + 1);
    return v;
  };
  // zero-padded copy of a per-channel vector (bias, LayerNorm affine, layer scale)
  auto pad_vec = [](size_t padded, int n) {
    return [padded, n](const auto* src, auto& out) {
      out.assign(padded, 0);
      for (int k = 0; k < n; ++k) out[k] = src[k];
    };
  };
  for (int i = 0; i < n_ops; ++i) {
    PackedOp op;
    op.d = ops[i];
    const ph_op_desc& d = op.d;
    auto widx_ok = [&](int k) { return k >= 0 && k < n_weights; };
    bool ok = true;
    switch (d.kind) {
      case PH_OP_POOL:
      case PH_OP_UPSAMPLE:
      case PH_OP_GELU:
      case PH_OP_GLOBAL_MAXPOOL:
        break;
      case PH_OP_SCALE_ADD: {
        if (!widx_ok(d.weight) || weight_numel[d.weight] != d.cout || d.cin0 != d.cout || d.src1 < 0) return fail("scale-add needs a (C) scale and two sources", i);
        ok = pack_upload(m, pad_vec(pad16(d.cout), d.cout), weights[d.weight], index_array(d.weight), &op.w_dev) == PH_OK;
        break;
      }
      case PH_OP_STEM: {
        if (d.ksize != 3 || d.cmid < 1 || d.cmid > 16 || d.cout < 1 || d.cout > 16 || (d.cin0 != 1 && d.cin0 != 3))
          return fail("fused stem needs kernel 3, 1 or 3 input channels and <= 16 filters", i);
        if (!widx_ok(d.weight) || !widx_ok(d.bias) || !widx_ok(d.weight2) || !widx_ok(d.bias2)) return fail("weight index out of range", i);
        if (weight_numel[d.weight] != (int64_t)d.cmid * d.cin0 * 9 || weight_numel[d.bias] != d.cmid ||
            weight_numel[d.weight2] != (int64_t)d.cout * d.cmid * 9 || weight_numel[d.bias2] != d.cout)
          return fail("stem weight size mismatch", i);
        auto pack_w0 = [&](const auto* w0, auto& p0) {
          p0.assign((size_t)9 * d.cin0 * 16, 0);
          for (int co = 0; co < d.cmid; ++co)
            for (int ci = 0; ci < d.cin0; ++ci)
              for (int tap = 0; tap < 9; ++tap) p0[((size_t)tap * d.cin0 + ci) * 16 + co] = w0[((size_t)co * d.cin0 + ci) * 9 + tap];
        };
        auto pack_w1 = [&](const auto* w1, auto& p1) {
          p1.assign((size_t)9 * 16 * 16, 0);
          for (int co = 0; co < d.cout; ++co)
            for (int ci = 0; ci < d.cmid; ++ci)
              for (int tap = 0; tap < 9; ++tap) p1[((size_t)tap * 16 + co) * 16 + ci] = w1[((size_t)co * d.cmid + ci) * 9 + tap];
        };
        ok = pack_upload(m, pack_w0, weights[d.weight], index_array(d.weight), &op.w_dev) == PH_OK &&
             pack_upload(m, pad_vec(16, d.cmid), weights[d.bias], index_array(d.bias), &op.b_dev) == PH_OK &&
             pack_upload(m, pack_w1, weights[d.weight2], index_array(d.weight2), &op.w2_dev) == PH_OK &&
             pack_upload(m, pad_vec(16, d.cout), weights[d.bias2], index_array(d.bias2), &op.b2_dev) == PH_OK;
        if (ok) {  // Winograd form of the second conv, derived on the device (refreshed by ph_model_set_params)
          float* w = nullptr;
          ok = hipMalloc(&w, 12 * 256 * sizeof(float)) == hipSuccess;
          if (ok) {
            m->allocs.push_back(w);
            ok = launch_stem_wino_pack(op.w2_dev, w, nullptr) == PH_OK;
            add_derived(m, DERIVED_WINO, op.w2_dev, w);  // (bn 0: the stem's form)
            op.w_wino_dev = w;
          }
        }
        if (ok) {  // ... and its F(2x2,3x3) form (the default)
          float* w = nullptr;
          ok = hipMalloc(&w, 16 * 256 * sizeof(float)) == hipSuccess;
          if (ok) {
            m->allocs.push_back(w);
            ok = launch_stem_wino2d_pack(op.w2_dev, w, nullptr) == PH_OK;
            add_derived(m, DERIVED_STEM_WINO2D, op.w2_dev, w);
            op.w_stem2_dev = w;
          }
        }
        break;
      }
      case PH_OP_CONV:
      case PH_OP_CONVT: {
        if (!widx_ok(d.weight) || !widx_ok(d.bias)) return fail("weight index out of range", i);
        if (weight_numel[d.bias] != d.cout) return fail("bias size mismatch", i);
        if (d.kind == PH_OP_CONVT && d.ksize != 3) return fail("transposed conv: only kernel 3 (stride 2, padding 1, output padding 1)", i);
        if (d.ksize != 3) {
          // kernel_size 5 / 7 / 9 (and the 7x7 convs of a stem block): k x k "same" conv as a k^2-tap row GEMM (mode 5); inference only
          if (!(d.ksize & 1) || d.ksize < 1 || d.ksize > 9) return fail("kernel_size must be odd and <= 9", i);
          if (weight_numel[d.weight] != (int64_t)(d.cin0 + d.cin1) * d.cout * d.ksize * d.ksize) return fail("weight size mismatch", i);
          const int coutp_k = pad16(d.cout);
          op.bn_g = gemm_choose_bn(coutp_k);
          auto pack_k = [&](const auto* w, auto& out) { pack_gemm(w, d.cout, d.cin0, d.cin1, d.ksize * d.ksize, op.bn_g, out); };
          ok = pack_upload(m, pack_k, weights[d.weight], index_array(d.weight), &op.w_gemm_dev) == PH_OK &&
               pack_upload(m, pad_vec((size_t)((coutp_k + op.bn_g - 1) / op.bn_g) * op.bn_g, d.cout), weights[d.bias], index_array(d.bias), &op.b_gemm_dev) == PH_OK;
          if (ok && d.kind == PH_OP_CONV) {  // data-gradient weights (training): the same k x k row GEMM on the flipped, in/out-swapped taps, one per concat source
            const int cin_total = d.cin0 + d.cin1;
            const int parts[2] = {d.cin0, d.cin1}, offs[2] = {0, d.cin0};
            int max_bn = 32;
            const std::vector<double> iwk = index_array(d.weight);
            for (int part = 0; part < 2 && ok; ++part) {
              if (parts[part] <= 0) continue;
              op.bn_dk[part] = gemm_choose_bn(pad16(parts[part]));
              max_bn = std::max(max_bn, op.bn_dk[part]);
              auto pack_dk = [&](const auto* w, auto& out) {
                std::remove_reference_t<decltype(out)> dw;
                dgrad_weight(w, d.cout, cin_total, offs[part], parts[part], dw, d.ksize);
                pack_gemm(dw.data(), parts[part], d.cout, 0, d.ksize * d.ksize, op.bn_dk[part], out);
              };
              ok = pack_upload(m, pack_dk, weights[d.weight], iwk, &op.wdk_gemm_dev[part]) == PH_OK;
            }
            if (ok) {
              std::vector<float> zb((size_t)pad16(std::max(d.cin0, d.cin1)) + 2 * max_bn, 0.f);
              ok = upload(m, zb, &op.zero_bias_dev) == PH_OK;
            }
          }
          break;
        }
        if (d.kind == PH_OP_CONVT && d.cin1 != 0) return fail("transposed conv takes one source", i);
        if (weight_numel[d.weight] != (int64_t)(d.cin0 + d.cin1) * d.cout * 9) return fail("weight size mismatch", i);
        const int coutp = pad16(d.cout);
        op.bn = choose_bn(coutp);
        const bool tr = d.kind == PH_OP_CONVT;
        const std::vector<double> iw = index_array(d.weight), ib = index_array(d.bias);
        auto pack_reg = [&](const auto* w, auto& out) { pack_conv(w, tr, d.cin0, d.cin1, d.cout, op.bn, out); };
        auto pack_dma = [&](const auto* w, auto& out) {
          std::remove_reference_t<decltype(out)> tmp;
          pack_conv(w, tr, d.cin0, d.cin1, d.cout, op.bn, tmp);
          repack_dma(tmp, op.bn, out);
        };
        ok = pack_upload(m, pack_reg, weights[d.weight], iw, &op.w_dev) == PH_OK && pack_upload(m, pack_dma, weights[d.weight], iw, &op.w_dma_dev) == PH_OK &&
             pack_upload(m, pad_vec((size_t)((coutp + op.bn - 1) / op.bn) * op.bn, d.cout), weights[d.bias], ib, &op.b_dev) == PH_OK;
        // Winograd F(2,3) weights of an N-tile-64 conv: a linear combination of taps, so not a gather of parameters --
        // computed on the device from the packed [tap] panels, again after every ph_model_set_params
        auto derive_wino = [&](const float* src, int cin_a, int cin_b, int cout_, int bn, float** dst) {
          if (bn != 64 && bn != 32) return true;
          const int panels = ((pad16(cout_) + bn - 1) / bn) * (pad16(cin_a) / 16 + (cin_b > 0 ? pad16(cin_b) / 16 : 0));
          float* w = nullptr;
          if (hipMalloc(&w, (size_t)wino_pack_floats(panels, bn) * sizeof(float)) != hipSuccess) return false;
          m->allocs.push_back(w);
          if (launch_wino_pack(src, w, panels, bn, nullptr) != PH_OK) return false;
          add_derived(m, DERIVED_WINO, src, w, panels, bn);
          *dst = w;
          return true;
        };
        if (ok && !tr) ok = derive_wino(op.w_dev, d.cin0, d.cin1, d.cout, op.bn, &op.w_wino_dev);
        // F(2x2,3x3) weights (conv3x3_wino2d_kernel, N tile 64): the forward conv's, and below the data-gradient convs'
        auto derive_wino2 = [&](const float* src, int cin_a, int cin_b, int cout_, int bn, float** dst) {
          if (bn != 64) return true;
          const int panels = ((pad16(cout_) + 63) / 64) * (pad16(cin_a) / 16 + (cin_b > 0 ? pad16(cin_b) / 16 : 0));
          float* w = nullptr;
          if (hipMalloc(&w, (size_t)wino2d_pack_floats(panels, 64) * sizeof(float)) != hipSuccess) return false;
          m->allocs.push_back(w);
          if (launch_wino2d_pack(src, w, panels, 64, nullptr) != PH_OK) return false;
          add_derived(m, DERIVED_WINO2D, src, w, panels, 64);
          *dst = w;
          return true;
        };
        if (ok && !tr) ok = derive_wino2(op.w_dev, d.cin0, d.cin1, d.cout, op.bn, &op.w_wino2_dev);
        if (ok && !tr && op.bn == 32 && coutp == 32 && pad16(d.cin0) + (d.cin1 > 0 ? pad16(d.cin1) : 0) >= 64) {
          // 32 output channels, K >= 64: a second packing with an N tile of 64 (rows 32 .. 63 zero) for the F(2x2,3x3) kernel's half-empty-tile form (conv_n32_wino2d)
          auto pack_64 = [&](const auto* w, auto& out) { pack_conv(w, false, d.cin0, d.cin1, d.cout, 64, out); };
          ok = pack_upload(m, pack_64, weights[d.weight], iw, &op.w_n64_dev) == PH_OK && pack_upload(m, pad_vec(64, d.cout), weights[d.bias], ib, &op.b_n64_dev) == PH_OK &&
               derive_wino2(op.w_n64_dev, d.cin0, d.cin1, d.cout, 64, &op.w_wino2_dev);
        }
        // F(4x4,3x3) weights (conv3x3_wino4_kernel) of the layers with many input channels: 4x the direct weights' bytes
        auto derive_wino4 = [&](const float* src, int cin_a, int cin_b, int cout_, int bn, float** dst) {
          if (bn != 64 || pad16(cin_a) + (cin_b > 0 ? pad16(cin_b) : 0) < 64) return true;  // (derived from 64 input channels on; which layers take the kernel is conv_wino4_min_cin + the time model)
          const int ntiles = (pad16(cout_) + 63) / 64, nchunks = pad16(cin_a) / 16 + (cin_b > 0 ? pad16(cin_b) / 16 : 0);
          float* w = nullptr;
          if (hipMalloc(&w, (size_t)wino4_pack_floats(ntiles, nchunks) * sizeof(float)) != hipSuccess) return false;
          m->allocs.push_back(w);
          if (launch_wino4_pack(src, w, pad16(cout_), nchunks, nullptr) != PH_OK) return false;
          add_derived(m, DERIVED_WINO4, src, w, pad16(cout_), nchunks);
          *dst = w;
          return true;
        };
        if (ok && !tr) ok = derive_wino4(op.w_dev, d.cin0, d.cin1, d.cout, op.bn, &op.w_wino4_dev);
        if (ok && !tr && op.w_n64_dev) ok = derive_wino4(op.w_n64_dev, d.cin0, d.cin1, d.cout, 64, &op.w_wino4_dev);  // (Cout 32, K >= 64: the N-tile-64 packing above; the kernel's waves of the empty N half skip their MFMAs)
        // wave-private F(2x2,3x3) weights (conv3x3_w16_kernel: 16 / 32 output channels, 16 / 32 input channels, one source): the forward
        // conv's, and below the data-gradient convs'
        auto derive_w16 = [&](const float* src, int cin_, int cout_, int bn, float** dst, int cin_b = 0) {
          const int cip = pad16(cin_), cibp = cin_b > 0 ? pad16(cin_b) : 0, cop = pad16(cout_);
          if (bn != 32 || !w16_shape_ok(cip, cibp, cop)) return true;
          const int chunks = (cip + cibp) / 16, nbs = cop / 16;
          float* w = nullptr;
          if (hipMalloc(&w, (size_t)w16_pack_floats(chunks, nbs) * sizeof(float)) != hipSuccess) return false;
          m->allocs.push_back(w);
          if (launch_w16_pack(src, w, chunks, nbs, nullptr) != PH_OK) return false;
          add_derived(m, DERIVED_W16, src, w, chunks, nbs);
          *dst = w;
          return true;
        };
        if (ok && !tr) ok = derive_w16(op.w_dev, d.cin0, d.cout, op.bn, &op.w_w16_dev, d.cin1);
        if (ok && !tr) {  // small-map F(2x2,3x3) weights (conv3x3_sm_kernel): 16/9 of the direct weights' bytes, every 3x3 conv
          const int nblocks = coutp / 16, chunks16 = pad16(d.cin0) / 16 + (d.cin1 > 0 ? pad16(d.cin1) / 16 : 0);
          float* w = nullptr;
          ok = hipMalloc(&w, (size_t)sm_pack_floats(nblocks, chunks16) * sizeof(float)) == hipSuccess;
          if (ok) {
            m->allocs.push_back(w);
            ok = launch_sm_pack(op.w_dev, w, nblocks, chunks16, op.bn, nullptr) == PH_OK;
            add_derived(m, DERIVED_SMALLMAP, op.w_dev, w, nblocks, chunks16).n_tiles = op.bn;
            op.w_sm_dev = w;
          }
        }
        if (ok && !tr) {  // row-GEMM form for feature maps too small for the 16x32-pixel tiles
          op.bn_g = gemm_choose_bn(coutp);
          auto pack_g = [&](const auto* w, auto& out) { pack_gemm(w, d.cout, d.cin0, d.cin1, 9, op.bn_g, out); };
          ok = pack_upload(m, pack_g, weights[d.weight], iw, &op.w_gemm_dev) == PH_OK &&
               pack_upload(m, pad_vec((size_t)((coutp + op.bn_g - 1) / op.bn_g) * op.bn_g, d.cout), weights[d.bias], ib, &op.b_gemm_dev) == PH_OK;
        }
        const bool c16 = d.kind == PH_OP_CONV && d.cin1 == 0 && d.cin0 <= 16 && d.cout <= 16;
        if (ok && c16) {
          auto pack_16 = [&](const auto* w, auto& out) { pack_c16(w, d.cout, d.cin0, out); };
          auto pack_16d = [&](const auto* w, auto& out) {
            std::remove_reference_t<decltype(out)> dw;
            dgrad_weight(w, d.cout, d.cin0, 0, d.cin0, dw);
            pack_c16(dw.data(), d.cin0, d.cout, out);
          };
          ok = pack_upload(m, pack_16, weights[d.weight], iw, &op.w16_dev) == PH_OK && pack_upload(m, pack_16d, weights[d.weight], iw, &op.wd16_dev) == PH_OK;
        }
        if (ok && tr) {
          // ConvTranspose2d(k3, s2, p1, op1): output (oy, ox) = (2y - 1 + ky, 2x - 1 + kx).  Even output rows see only ky = 1
          // (input row y), odd rows ky = 0 (input row y + 1) and ky = 2 (row y) -- likewise in x: four output phases with
          // 1, 2, 2, 4 taps.  Each phase is one row GEMM over the input grid (mode 3) whose tap t reads input pixel
          // (y + dy, x + dx); weights per phase: wp[co][ci][t] = Wt[ci][co][ky(t)][kx(t)].
          op.bn_t = gemm_choose_bn(coutp);
          const size_t npad_t = (size_t)((coutp + op.bn_t - 1) / op.bn_t) * op.bn_t;
          for (int ph = 0; ph < 4 && ok; ++ph) {
            const int py = ph >> 1, px = ph & 1, nt = (1 + py) * (1 + px);
            auto pack_p = [&](const auto* w, auto& out) {
              std::remove_reference_t<decltype(out)> wp((size_t)d.cout * d.cin0 * nt);
              for (int t = 0; t < nt; ++t) {
                const int ty = px ? t >> 1 : t, tx = px ? t & 1 : 0;
                const int ky = py ? 2 * ty : 1, kx = px ? 2 * tx : 1;  // tap t reads (y + 1 - ty, x + 1 - tx): ky = 0 <-> dy = 1
                for (int co = 0; co < d.cout; ++co)
                  for (int ci = 0; ci < d.cin0; ++ci) wp[((size_t)co * d.cin0 + ci) * nt + t] = w[(((size_t)ci * d.cout + co) * 3 + ky) * 3 + kx];
              }
              pack_gemm(wp.data(), d.cout, d.cin0, 0, nt, op.bn_t, out);
            };
            ok = pack_upload(m, pack_p, weights[d.weight], iw, &op.wt_phase_dev[ph]) == PH_OK;
          }
          if (ok) ok = pack_upload(m, pad_vec(npad_t, d.cout), weights[d.bias], ib, &op.bt_dev) == PH_OK;
          if (ok && d.weight2 >= 0) {  // folded BatchNorm (eval): y = act(scale * (conv + bias) + shift)
            if (!widx_ok(d.weight2) || !widx_ok(d.bias2) || weight_numel[d.weight2] != d.cout || weight_numel[d.bias2] != d.cout) return fail("transposed conv: scale / shift must be (cout)", i);
            ok = pack_upload(m, pad_vec(npad_t, d.cout), weights[d.weight2], index_array(d.weight2), &op.wt_scale_dev) == PH_OK &&
                 pack_upload(m, pad_vec(npad_t, d.cout), weights[d.bias2], index_array(d.bias2), &op.wt_shift_dev) == PH_OK;
          }
          if (ok) {  // data gradient = Conv2d(dY, Wt as (out = cin0, in = cout, 3, 3), stride 2, pad 1): the ConvTranspose2d weight as it lies in memory
            const int cinp = pad16(d.cin0);
            op.bn_td = gemm_choose_bn(cinp);
            auto pack_dg = [&](const auto* w, auto& out) { pack_gemm(w, d.cin0, d.cout, 0, 9, op.bn_td, out); };
            std::vector<float> zb((size_t)cinp + 128, 0.f);
            ok = pack_upload(m, pack_dg, weights[d.weight], iw, &op.wt_dgrad_dev) == PH_OK && upload(m, zb, &op.zero_bias_dev) == PH_OK;
          }
        }
        if (ok && d.kind == PH_OP_CONV) {  // data-gradient weights (training)
          const int cin_total = d.cin0 + d.cin1;
          const int parts[2] = {d.cin0, d.cin1}, offs[2] = {0, d.cin0};
          int max_bn = 32;
          for (int part = 0; part < 2 && ok; ++part) {
            if (parts[part] <= 0) continue;
            op.bn_d[part] = choose_bn(pad16(parts[part]));
            max_bn = std::max(max_bn, op.bn_d[part]);
            auto pack_d = [&](const auto* w, auto& out) {
              std::remove_reference_t<decltype(out)> dw;
              dgrad_weight(w, d.cout, cin_total, offs[part], parts[part], dw);
              pack_conv(dw.data(), false, d.cout, 0, parts[part], op.bn_d[part], out);
            };
            auto pack_dd = [&](const auto* w, auto& out) {
              std::remove_reference_t<decltype(out)> tmp;
              pack_d(w, tmp);
              repack_dma(tmp, op.bn_d[part], out);
            };
            ok = pack_upload(m, pack_d, weights[d.weight], iw, &op.wd_dev[part]) == PH_OK &&
                 pack_upload(m, pack_dd, weights[d.weight], iw, &op.wd_dma_dev[part]) == PH_OK &&
                 derive_wino(op.wd_dev[part], d.cout, 0, parts[part], op.bn_d[part], &op.wd_wino_dev[part]) &&
                 derive_wino2(op.wd_dev[part], d.cout, 0, parts[part], op.bn_d[part], &op.wd_wino2_dev[part]) &&
                 derive_w16(op.wd_dev[part], d.cout, parts[part], op.bn_d[part], &op.wd_w16_dev[part]) &&
                 derive_wino4(op.wd_dev[part], d.cout, 0, parts[part], op.bn_d[part], &op.wd_wino4_dev[part]);
          }
          if (ok) {
            std::vector<float> zb((size_t)pad16(std::max(d.cin0, d.cin1)) + max_bn, 0.f);
            ok = upload(m, zb, &op.zero_bias_dev) == PH_OK;
          }
        }
        break;
      }
      case PH_OP_INPUT_CONV:
      case PH_OP_PATCH_STEM: {
        // [tap][ci][Cp] from OIHW (cout, cin, k, k); the patch stem (k x k, stride = cmid, padding 1) shares the layout
        if (!widx_ok(d.weight) || !widx_ok(d.bias)) return fail("weight index out of range", i);
        if (weight_numel[d.bias] != d.cout) return fail("bias size mismatch", i);
        if (d.kind == PH_OP_INPUT_CONV && (!(d.ksize & 1) || d.ksize < 1 || d.ksize > 9)) return fail("kernel_size must be odd and <= 9", i);
        if (d.kind == PH_OP_PATCH_STEM && (d.ksize < 2 || d.ksize > 8 || d.cmid < 1 || d.cmid > d.ksize)) return fail("patch stem needs 2 <= kernel <= 8 and 1 <= stride <= kernel", i);
        if (d.kind == PH_OP_PATCH_STEM && (d.flags & PH_FLAG_PAD0_NORM) && (d.cin0 < 1 || d.cin0 > 4)) return fail("a padding-0 patch stem with input statistics takes 1..4 input channels", i);
        const int kk = d.ksize * d.ksize;
        if (weight_numel[d.weight] != (int64_t)d.cin0 * d.cout * kk) return fail("weight size mismatch", i);
        const int coutp = pad16(d.cout);
        auto pack_in = [&](const auto* w, auto& out) {
          out.assign((size_t)kk * d.cin0 * coutp, 0);
          for (int co = 0; co < d.cout; ++co)
            for (int ci = 0; ci < d.cin0; ++ci)
              for (int tap = 0; tap < kk; ++tap) out[((size_t)tap * d.cin0 + ci) * coutp + co] = w[((size_t)co * d.cin0 + ci) * kk + tap];
        };
        ok = pack_upload(m, pack_in, weights[d.weight], index_array(d.weight), &op.w_dev) == PH_OK &&
             pack_upload(m, pad_vec(coutp, d.cout), weights[d.bias], index_array(d.bias), &op.b_dev) == PH_OK;
        break;
      }
      case PH_OP_HEAD: {
        if (!widx_ok(d.weight) || !widx_ok(d.bias)) return fail("weight index out of range", i);
        if (weight_numel[d.bias] != d.cout) return fail("bias size mismatch", i);
        if (weight_numel[d.weight] != (int64_t)d.cin0 * d.cout) return fail("weight size mismatch", i);
        if (d.out_index < 0 || d.out_index >= n_outputs) return fail("bad out_index", i);
        const int cp = pad16(d.cin0);
        auto pack_head = [&](const auto* w, auto& out) {
          out.assign((size_t)d.cout * cp, 0);
          for (int co = 0; co < d.cout; ++co)
            for (int ci = 0; ci < d.cin0; ++ci) out[(size_t)co * cp + ci] = w[(size_t)co * d.cin0 + ci];
        };
        ok = pack_upload(m, pack_head, weights[d.weight], index_array(d.weight), &op.w_dev) == PH_OK &&
             pack_upload(m, pad_vec(d.cout, d.cout), weights[d.bias], index_array(d.bias), &op.b_dev) == PH_OK;
        break;
      }
      case PH_OP_DWCONV: {
        // (C, 1, 7, 7) -> [tap][Cp]
        if (!widx_ok(d.weight) || !widx_ok(d.bias)) return fail("weight index out of range", i);
        if (d.ksize != 7 || d.cin0 != d.cout) return fail("depthwise conv must be 7x7 with cin == cout", i);
        if (weight_numel[d.weight] != (int64_t)d.cout * 49 || weight_numel[d.bias] != d.cout) return fail("weight size mismatch", i);
        const int cp = pad16(d.cout);
        auto pack_dw = [&](const auto* w, auto& out) {
          out.assign((size_t)49 * cp, 0);
          for (int c = 0; c < d.cout; ++c)
            for (int tap = 0; tap < 49; ++tap) out[(size_t)tap * cp + c] = w[(size_t)c * 49 + tap];
        };
        auto pack_dw_flip = [&](const auto* w, auto& out) {  // data gradient = the same kernel on the spatially flipped taps
          out.assign((size_t)49 * cp, 0);
          for (int c = 0; c < d.cout; ++c)
            for (int tap = 0; tap < 49; ++tap) out[(size_t)(48 - tap) * cp + c] = w[(size_t)c * 49 + tap];
        };
        ok = pack_upload(m, pack_dw, weights[d.weight], index_array(d.weight), &op.w_dev) == PH_OK &&
             pack_upload(m, pad_vec(cp, d.cout), weights[d.bias], index_array(d.bias), &op.b_dev) == PH_OK &&
             pack_upload(m, pack_dw_flip, weights[d.weight], index_array(d.weight), &op.dw_flip_dev) == PH_OK;
        break;
      }
      case PH_OP_LAYERNORM: {
        if (!widx_ok(d.weight) || !widx_ok(d.bias)) return fail("weight index out of range", i);
        if (d.cin0 != d.cout || weight_numel[d.weight] != d.cout || weight_numel[d.bias] != d.cout) return fail("LayerNorm affine size mismatch", i);
        const int cp = pad16(d.cout);
        ok = pack_upload(m, pad_vec(cp, d.cout), weights[d.weight], index_array(d.weight), &op.w_dev) == PH_OK &&
             pack_upload(m, pad_vec(cp, d.cout), weights[d.bias], index_array(d.bias), &op.b_dev) == PH_OK;
        break;
      }
      case PH_OP_GRN: {
        if (!widx_ok(d.weight) || !widx_ok(d.bias)) return fail("weight index out of range", i);
        if (d.cin0 != d.cout || d.src0 < 0 || weight_numel[d.weight] != d.cout || weight_numel[d.bias] != d.cout) return fail("GRN needs a (C) weight and bias", i);
        const int cp = pad16(d.cout);
        ok = pack_upload(m, pad_vec(cp, d.cout), weights[d.weight], index_array(d.weight), &op.w_dev) == PH_OK &&
             pack_upload(m, pad_vec(cp, d.cout), weights[d.bias], index_array(d.bias), &op.b_dev) == PH_OK;
        break;
      }
      case PH_OP_PATCH_MERGE: {
        if (!widx_ok(d.weight) || !widx_ok(d.bias)) return fail("weight index out of range", i);
        if (d.cout != 4 * d.cin0 || (d.cin0 & 15) || weight_numel[d.weight] != d.cout || weight_numel[d.bias] != d.cout)
          return fail("patch merge needs a channel count that is a multiple of 16 and a (4C) LayerNorm affine", i);
        ok = pack_upload(m, pad_vec(d.cout, d.cout), weights[d.weight], index_array(d.weight), &op.w_dev) == PH_OK &&
             pack_upload(m, pad_vec(d.cout, d.cout), weights[d.bias], index_array(d.bias), &op.b_dev) == PH_OK;
        break;
      }
      case PH_OP_WINDOW_ATTN: {
        // weight = relative_position_bias_table ((2w - 1)^2, heads) -> head-major; bias = qkv.bias (3C): the q, k, v of a padded token
        if (!widx_ok(d.weight) || !widx_ok(d.bias)) return fail("weight index out of range", i);
        const int heads = d.cin1, rel = (2 * d.ksize - 1) * (2 * d.ksize - 1);
        if (d.ksize < 2 || d.ksize > 8) return fail("window attention needs 2 <= window_size <= 8", i);
        if (heads < 1 || d.cout != heads * 32 || d.cin0 != 3 * d.cout) return fail("window attention needs head dimension 32 and a (3C) qkv source", i);
        if (d.cmid < 0 || d.cmid >= d.ksize) return fail("window attention shift must be smaller than the window", i);
        if (weight_numel[d.weight] != (int64_t)rel * heads || weight_numel[d.bias] != d.cin0) return fail("weight size mismatch", i);
        auto pack_tbl = [&](const auto* w, auto& out) {
          out.assign((size_t)rel * heads, 0);
          for (int r = 0; r < rel; ++r)
            for (int a = 0; a < heads; ++a) out[(size_t)a * rel + r] = w[(size_t)r * heads + a];
        };
        ok = pack_upload(m, pack_tbl, weights[d.weight], index_array(d.weight), &op.w_dev) == PH_OK &&
             pack_upload(m, pad_vec(d.cin0, d.cin0), weights[d.bias], index_array(d.bias), &op.b_dev) == PH_OK;
        break;
      }
      case PH_OP_LINEAR:
      case PH_OP_PATCH_CONV: {
        const bool no_bias = d.kind == PH_OP_LINEAR && d.bias == -1;  // Linear(bias=False): Swin's patch-merging reduction
        if (!widx_ok(d.weight) || !(widx_ok(d.bias) || no_bias)) return fail("weight index out of range", i);
        const int segs = d.kind == PH_OP_PATCH_CONV ? 4 : 1;
        if (d.kind == PH_OP_PATCH_CONV && d.ksize != 2) return fail("patch conv must be 2x2 stride 2", i);
        if (weight_numel[d.weight] != (int64_t)d.cin0 * d.cout * segs || (!no_bias && weight_numel[d.bias] != d.cout)) return fail("weight size mismatch", i);
        if ((d.flags & PH_FLAG_RESIDUAL) && ((d.flags & PH_FLAG_SCALE_RESIDUAL) || d.src1 < 0)) return fail("residual epilogue needs a residual source and no layer scale", i);
        const int coutp = pad16(d.cout);
        op.bn = gemm_choose_bn(coutp);
        const size_t npad = (size_t)((coutp + op.bn - 1) / op.bn) * op.bn;
        auto pack_g = [&](const auto* w, auto& out) { pack_gemm(w, d.cout, d.cin0, 0, segs, op.bn, out); };
        ok = pack_upload(m, pack_g, weights[d.weight], index_array(d.weight), &op.w_dma_dev) == PH_OK;
        if (ok && no_bias) {
          std::vector<float> zb(npad, 0.f);  // (not a parameter: nothing in the arena maps onto it)
          ok = upload(m, zb, &op.b_dev) == PH_OK;
        } else if (ok) {
          ok = pack_upload(m, pad_vec(npad, d.cout), weights[d.bias], index_array(d.bias), &op.b_dev) == PH_OK;
        }
        if (ok && d.kind == PH_OP_LINEAR && (d.flags & PH_FLAG_GELU) && cnblock_mlp_fits(d.cin0, pad16(d.cin0), d.cout)) {  // inference programs: the first Linear of a CNBlock MLP ...
          auto pack_1 = [&](const auto* w, auto& out) { pack_mlp_w1(w, d.cin0, out); };
          ok = pack_upload(m, pack_1, weights[d.weight], index_array(d.weight), &op.w_mlp_dev) == PH_OK;
        } else if (ok && d.kind == PH_OP_LINEAR && (d.flags & PH_FLAG_SCALE_RESIDUAL) && cnblock_mlp_fits(d.cout, pad16(d.cout), d.cin0)) {  // ... and the second
          auto pack_2 = [&](const auto* w, auto& out) { pack_mlp_w2(w, d.cout, out); };
          ok = pack_upload(m, pack_2, weights[d.weight], index_array(d.weight), &op.w_mlp_dev) == PH_OK;
        }
        if (ok) {  // data-gradient weights (training): dX = dY * W, one transposed matrix per tap, + a zero bias
          const int cinp = pad16(d.cin0);
          op.bn_dg = gemm_choose_bn(cinp);
          for (int tap = 0; tap < segs && ok; ++tap) {
            auto pack_t = [&](const auto* w, auto& out) {
              std::remove_reference_t<decltype(out)> wt((size_t)d.cin0 * d.cout);
              for (int co = 0; co < d.cout; ++co)
                for (int ci = 0; ci < d.cin0; ++ci) wt[(size_t)ci * d.cout + co] = w[((size_t)co * d.cin0 + ci) * segs + tap];
              pack_gemm(wt.data(), d.cin0, d.cout, 0, 1, op.bn_dg, out);
            };
            ok = pack_upload(m, pack_t, weights[d.weight], index_array(d.weight), &op.wd_gemm_dev[tap]) == PH_OK;
          }
          if (ok) {
            std::vector<float> zb((size_t)cinp + 128, 0.f);
            ok = upload(m, zb, &op.zero_bias_dev) == PH_OK;
          }
        }
        if (ok) {  // fp16 image for gemm_f16_kernel (plain fp16 precision), derived on the device; refreshed by ph_model_set_params
          const int coutp32 = fmt_cpad(FMT_F16, d.cout), cinp32 = fmt_cpad(FMT_F16, d.cin0);
          void* w = nullptr;
          ok = hipMalloc(&w, (size_t)gemm_f16_weight_image_halves(coutp32, cinp32, segs) * 2) == hipSuccess;
          if (ok) {
            m->allocs.push_back(w);
            ok = launch_gemm_f16_weight_image(op.w_dma_dev, w, d.cout, d.cin0, coutp32, cinp32, segs, op.bn, nullptr) == PH_OK;
            DerivedBuffer& db = add_derived(m, DERIVED_GEMM_F16_IMAGE, op.w_dma_dev, static_cast<float*>(w), d.cout, op.bn);
            db.n_tiles = d.cin0;
            db.chunks0 = segs;
            op.w_cnx_f16_dev = w;
          }
        }
        if (ok && d.kind == PH_OP_LINEAR && (d.flags & PH_FLAG_RESIDUAL) && !no_bias && i > 0 && ops[i - 1].kind == PH_OP_GRN && ops[i - 1].dst == d.src0 && ops[i - 1].cout == d.cin0 &&
            widx_ok(ops[i - 1].bias) && weight_numel[ops[i - 1].bias] == d.cin0) {
          // fused GRN plan: W2 (s x + grn.bias) + b2 = (W2 diag(s)) x + (W2 grn.bias + b2); the second term is constant per set of parameters (ph_model_set_params recomputes it on the device, bit for bit this sum: launch_grn_fold_bias)
          std::vector<float> fb(npad, 0.f);
          const float* w2 = weights[d.weight];
          const float* gb = weights[ops[i - 1].bias];
          for (int co = 0; co < d.cout; ++co) {
            double acc = weights[d.bias][co];
            for (int ci = 0; ci < d.cin0; ++ci) acc += (double)w2[(size_t)co * d.cin0 + ci] * (double)gb[ci];
            fb[co] = (float)acc;
          }
          ok = upload(m, fb, &op.b_grn_dev) == PH_OK;
        }
        if (ok && (d.flags & PH_FLAG_SCALE_RESIDUAL)) {
          if (!widx_ok(d.weight2) || weight_numel[d.weight2] != d.cout || d.src1 < 0) return fail("layer-scale epilogue needs weight2 (C) and a residual source", i);
          ok = pack_upload(m, pad_vec(npad, d.cout), weights[d.weight2], index_array(d.weight2), &op.w2_dev) == PH_OK;
        }
        break;
      }
      default:
        return fail("unknown op kind", i);
    }
    if (!ok) {
      ph_model_destroy(m);
      return nullptr;
    }
    m->ops.push_back(op);
  }
  if (!m->derived.empty() && hipDeviceSynchronize() != hipSuccess) {  // the derived buffers were computed on the null stream
    set_error("ph_model_create: device synchronisation failed");
    ph_model_destroy(m);
    return nullptr;
  }
  return m;
}

void ph_model_destroy(ph_model* m) {
  if (!m) return;
  for (void* p : m->allocs) (void)hipFree(p);
  for (hipEvent_t e : m->ev) (void)hipEventDestroy(e);
  for (hipEvent_t e : m->bwd_ev) (void)hipEventDestroy(e);
  for (hipEvent_t e : m->comm_events_owned) (void)hipEventDestroy(e);
  delete m;
}

int64_t ph_model_workspace_bytes(const ph_model* m, int32_t batch, int32_t height, int32_t width) {
  if (!m || batch <= 0 || height <= 0 || width <= 0) {
    set_error("ph_model_workspace_bytes: bad arguments");
    return PH_E_INVALID;
  }
  Plan plan;
  int rc = build_plan(m, batch, height, width, plan, forward_format(m));
  if (rc != PH_OK) return rc;
  return plan.total;
}

int ph_model_output_shape(const ph_model* m, int32_t out_index, int32_t height, int32_t width, int32_t* c, int32_t* h, int32_t* w) {
  PH_REQUIRE(m && c && h && w, "ph_model_output_shape: null argument");
  Plan plan;
  int rc = build_plan(m, 1, height, width, plan);
  if (rc != PH_OK) return rc;
  for (const PackedOp& op : m->ops)
    if (op.d.kind == PH_OP_HEAD && op.d.out_index == out_index) {
      *c = op.d.cout;
      *h = plan.slots[op.d.src0].h;
      *w = plan.slots[op.d.src0].w;
      return PH_OK;
    }
  set_error("no head writes output %d", out_index);
  return PH_E_INVALID;
}

int32_t ph_op_desc_size(void) { return (int32_t)sizeof(ph_op_desc); }

int ph_debug_split_plan(int32_t B, int32_t H, int32_t W, int32_t cin_padded, int32_t cout_padded, int32_t splitk, int32_t n_cu, int64_t* out4) {
  PH_REQUIRE(out4 && B > 0 && H > 0 && W > 0 && cin_padded > 0 && cout_padded > 0 && n_cu > 0 && (cin_padded % 16) == 0 && (cout_padded % 16) == 0, "ph_debug_split_plan: bad arguments");
  out4[0] = wino2d_ksplit_shape(B, H, W, cin_padded, cout_padded, splitk, n_cu);
  out4[1] = ((H & 3) || (W & 3)) ? 1 : wino4_ksplit_shape(B, H, W, cin_padded, cout_padded, splitk, n_cu);
  out4[2] = wino2d_split_scratch_bytes(B, H, W, cin_padded, cout_padded, splitk, n_cu) / 1024;
  out4[3] = wino4_split_scratch_bytes(B, H, W, cin_padded, cout_padded, splitk, n_cu) / 1024;
  return PH_OK;
}

namespace {
struct OptionRef {
  const char* key;
  int* i;
  double* d;
};
// every tunable of a handle; defaults are the measured-best variants (DESIGN.md, appendix "handle options")
std::vector<OptionRef> option_table(ph_model* m) {
  return {
      {"conv_wino", &m->conv_wino, nullptr},            // 1 Winograd F(2,3) 3x3 kernels, 2 only N-tile-64 layers, 0 direct 9-tap kernels
      {"conv_w16", &m->conv_w16, nullptr},              // 1: Cout-32 / Cin-16-or-32 3x3 convs on the wave-private F(2x2,3x3) kernel; 0: F(2,3) along x
      {"conv_wino2d", &m->conv_wino2d, nullptr},        // 1: N-tile-64 3x3 convs on the F(2x2,3x3) kernel; 0: F(2,3) along x only
      {"conv_wino4", &m->conv_wino4, nullptr},          // K-heavy 3x3 convs on the F(4x4,3x3) kernel: 1 inference plans, 2 every plan (both: where estimated faster), 3 every plan wherever it fits, 0 never
      {"conv_wino4_min_cin", &m->conv_wino4_min_cin, nullptr},  // padded input channels from which a layer takes it
      {"conv_n32_wino2d", &m->conv_n32_wino2d, nullptr},  // Cout-32 / K >= 64 layers on the F(2x2,3x3) kernel with a half-empty N tile (0: the N-tile-32 F(2,3) kernel)
      {"conv_splitk_finish", &m->conv_splitk_finish, nullptr},  // 0: the split-K second stage as a launch of its own (A/B, tests)
      {"grn_fuse", &m->grn_fuse, nullptr},                // ConvNeXtV2 blocks on the fused GRN plan: 1 sums of squares from the first Linear's epilogue + per-sample scaled weights for the second; 0 (default, measured faster) two GRN launches
      {"pretrained_train", &m->pretrained_train, nullptr},  // 1: ph_model_backward accepts a ConvNeXtV2 program (GRN backward, weight gradient of the padding-0 stem); 0 (default) refuses its PH_FLAG_NO_TRAIN ops
      {"bwd_frozen_ops", &m->bwd_frozen_ops, nullptr},      // the first n ops get no backward step (frozen encoder); 0 (default) none
      {"mlp_fuse", &m->mlp_fuse, nullptr},              // inference plans: CNBlock's two Linears (+ GELU, layer scale, residual) in one launch (cnblock_mlp_kernel)
      {"block_fuse", &m->block_fuse, nullptr},          // plain fp16, inference plans: the two convs of a 32-channel encoder block in one launch (block2_c32_f16_kernel)
      {"stem_f16mfma", &m->stem_f16mfma, nullptr},      // plain fp16: the fused first block with BOTH convs on the fp16 matrix pipe (stem_f16_kernel) instead of stem_fused_kernel<CIN, 3>
      {"upsample_f16math", &m->upsample_f16math, nullptr},  // a bilinear x2 folded into conv3x3_f16_rows_kernel blends in packed fp16 arithmetic (1) or in fp32 as upsample2x_fmt_kernel does (0)
      {"conv_f16_rows", &m->conv_f16_rows, nullptr},    // plain-fp16 precision: conv3x3_f16_rows_kernel 0 never, 1 where its plan is estimated faster than conv3x3_f16_persist_kernel, 2 wherever the shape fits
      {"conv_f16_rows_pin", &m->conv_f16_rows_pin, nullptr},  // tests: the one (R, Wt, MG) tile f16_rows_plan considers, packed R | Wt << 8 | MG << 16 (0: the search)
      {"conv_smallmap", &m->conv_smallmap, nullptr},    // conv3x3_sm_kernel for small maps at small batches: 0 never, 1 where estimated faster (inference plans, conv_splitk = 1), 2 wherever the shape fits
      {"conv_splitk", &m->conv_splitk, nullptr},        // split K on the F(2x2,3x3) kernel for layers with fewer work units than CUs: 0 never, 1 where estimated faster, n >= 2 force n slices
      {"upsample_fold", &m->upsample_fold, nullptr},    // bilinear x2 folded into the F(4x4,3x3) input transform of the conv that consumes it
      {"stem_wino", &m->stem_wino, nullptr},            // second conv of the fused stem in Winograd form
      {"dgrad_wino", &m->dgrad_wino, nullptr},          // 0: direct 9-tap kernels for the backward's data-gradient convs
      {"conv_dma", &m->use_dma, nullptr},               // 0: register-staged 3x3 kernel instead of the LDS-DMA family
      {"conv_dma32", &m->dma32, nullptr},               // 0: Cout <= 48 layers on the register-staged kernel
      {"conv_persist", &m->conv_persist, nullptr},      // 0: one pixel tile per workgroup
      {"conv_c16", &m->conv_c16, nullptr},              // 0: 16 -> 16 channel layers on the generic kernel
      {"conv_dma_stagger", &m->dma_stagger, nullptr},   // 0: SIMD-partner waves issue DMA pieces at the same step
      {"fuse_gelu_fwd", &m->fuse_gelu_fwd, nullptr},
      {"fuse_gelu_bwd", &m->fuse_gelu_bwd, nullptr},
      {"dw_ln_fuse", &m->dw_ln_fuse, nullptr},          // ConvNeXt inference: LayerNorm fused into the depthwise 7x7 kernel
      {"head_fuse", &m->head_fuse, nullptr},            // a 1x1 head on a 64-channel conv output is computed in that conv's F(2x2,3x3) epilogue
      {"pool_peephole", &m->pool_peephole, nullptr},    // unfused programs: a conv whose next op pools its output writes the pooled tensor from its epilogue
      {"mask_fold", &m->mask_fold, nullptr},            // ReLU mask applied by the pool backward that completes a conv output's gradient
      {"wgrad_wino", &m->wgrad_wino, nullptr},          // 3x3 weight gradients: 1 Winograd F(2x2,3x3) domain, 0 direct nine-tap kernel
      {"wgrad_rows", &m->wgrad_rows, nullptr},          // 0 32x32-tile wgrad kernel, 1 auto, 2 nine row-wgrad GEMMs
      {"workspace_reuse", &m->workspace_reuse, nullptr},  // 1: activation slots share memory once their last reader has run (inference programs only); 2: that plan's routing and fusions, every slot in its own range (tests: ph_model_read_slot across a fused launch)
      {"convt_one_launch", &m->convt_one_launch, nullptr},  // 1: the four output-phase GEMMs of a transposed conv in one launch (grid.y = phase); 0: four launches
      {"convt_phase", &m->convt_phase, nullptr},        // 0: transposed convs by zero-stuffing + 3x3 conv (4x the FLOPs; A/B reference)
      {"convnext_f16", &m->convnext_f16, nullptr},      // 1: under conv_precision 2 a ConvNeXt program runs whole in plain fp16 (0: exact fp32 whatever the precision)
      {"swint_f16", &m->swint_f16, nullptr},            // 1: under conv_precision 2 a Swin program runs whole in plain fp16 (0: exact fp32 whatever the precision); independent of convnext_f16
      {"conv_precision", &m->conv_precision, nullptr},  // 0 exact fp32 MFMA, 1 split-fp16 MFMA (22-bit products), 2 plain fp16 (autocast-equivalent)
      {"gemm_late_split", &m->gemm_late_split, nullptr},
      {"gemm_persist2", &m->gemm_persist2, nullptr},
      {"conv_gemm_fill", nullptr, &m->gemm_fill_threshold},            // tile fill below which a 3x3 conv runs as a row GEMM (0 disables)
      {"conv_gemm_fill_wino", nullptr, &m->gemm_fill_threshold_wino},  // ... when the halo kernel is the Winograd one
      {"conv_gemm_fill_wino2d", nullptr, &m->gemm_fill_threshold_wino2d},  // ... when it is the F(2x2,3x3) kernel (16x16-pixel tiles)
  };
}
}  // namespace

int ph_model_set_input_norm(ph_model* m, const float* mean, const float* std, int32_t n) {
  PH_REQUIRE(m && mean && std && n >= 1 && n <= 4, "ph_model_set_input_norm: needs 1..4 channels");
  for (int c = 0; c < n; ++c) PH_REQUIRE(std[c] != 0.f && std::isfinite(std[c]) && std::isfinite(mean[c]), "ph_model_set_input_norm: channel %d has a zero or non-finite statistic", c);
  for (int c = 0; c < n; ++c) {
    m->in_mean[c] = mean[c];
    m->in_std[c] = std[c];
  }
  return PH_OK;
}

int ph_model_set_option(ph_model* m, const char* key, double value) {
  PH_REQUIRE(m && key, "ph_model_set_option: null argument");
  for (const OptionRef& o : option_table(m))
    if (!strcmp(o.key, key)) {
      if (o.i) *o.i = (int)value;
      if (o.d) *o.d = (!strcmp(key, "conv_gemm_fill_wino") || !strcmp(key, "conv_gemm_fill_wino2d")) ? std::max(value, 1e-3) : value;
      return PH_OK;
    }
  set_error("ph_model_set_option: unknown option '%s'", key);
  return PH_E_INVALID;
}

int ph_model_get_option(const ph_model* m, const char* key, double* value) {
  PH_REQUIRE(m && key && value, "ph_model_get_option: null argument");
  for (const OptionRef& o : option_table(const_cast<ph_model*>(m)))
    if (!strcmp(o.key, key)) {
      *value = o.i ? (double)*o.i : *o.d;
      return PH_OK;
    }
  set_error("ph_model_get_option: unknown option '%s'", key);
  return PH_E_INVALID;
}

int ph_model_set_profiling(ph_model* m, int32_t enabled) {
  PH_REQUIRE(m, "ph_model_set_profiling: null model");
  if (enabled && m->ev.empty()) {
    m->ev.resize(m->ops.size() + 1);
    for (auto& e : m->ev) PH_HIP_CHECK(hipEventCreate(&e));
  }
  if (enabled == 1 || m->op_ms.size() != m->ops.size()) {
    m->op_ms.assign(m->ops.size(), 0.0);
    m->profiled_forwards = 0;
    m->events_pending = false;
  }
  m->profiling = enabled != 0;
  return PH_OK;
}

int ph_model_profile_read(ph_model* m, double* op_ms, int32_t n_ops, int32_t* n_forwards) {
  PH_REQUIRE(m && op_ms && n_forwards, "ph_model_profile_read: null argument");
  PH_REQUIRE(n_ops == (int32_t)m->ops.size(), "ph_model_profile_read: model has %d ops", (int)m->ops.size());
  int rc = drain_events(m);
  if (rc != PH_OK) return rc;
  for (int i = 0; i < n_ops; ++i) op_ms[i] = i < (int)m->op_ms.size() ? m->op_ms[i] : 0.0;
  *n_forwards = m->profiled_forwards;
  return PH_OK;
}

int ph_model_last_kernels(const ph_model* m, int32_t* codes, int32_t n_ops) {
  PH_REQUIRE(m && codes, "ph_model_last_kernels: null argument");
  PH_REQUIRE(n_ops == (int32_t)m->ops.size(), "ph_model_last_kernels: model has %d ops", (int)m->ops.size());
  for (int i = 0; i < n_ops; ++i) codes[i] = i < (int)m->last_variant.size() ? m->last_variant[i] : PH_KV_NONE;
  return PH_OK;
}

int ph_model_last_rows_plans(const ph_model* m, int32_t* quad, int32_t n_ops) {
  PH_REQUIRE(m && quad, "ph_model_last_rows_plans: null argument");
  PH_REQUIRE(n_ops == (int32_t)m->ops.size(), "ph_model_last_rows_plans: model has %d ops", (int)m->ops.size());
  for (int i = 0; i < 4 * n_ops; ++i) quad[i] = i < (int)m->last_rows_plan.size() ? m->last_rows_plan[i] : 0;
  return PH_OK;
}

int ph_model_last_ranges(const ph_model* m, int64_t* rows, int32_t max_rows, int32_t* n_rows) {
  PH_REQUIRE(m && n_rows && max_rows >= 0 && (rows || max_rows == 0), "ph_model_last_ranges: bad arguments");
  *n_rows = (int32_t)m->last_ranges.size();
  for (int i = 0; i < max_rows && i < *n_rows; ++i) {
    const RangeRec& r = m->last_ranges[i];
    rows[6 * i] = r.op;
    rows[6 * i + 1] = r.launch;
    rows[6 * i + 2] = r.is_dst;
    rows[6 * i + 3] = r.slot;
    rows[6 * i + 4] = r.offset;
    rows[6 * i + 5] = r.bytes;
  }
  return PH_OK;
}

int ph_model_set_clock_probe(ph_model* m, void* buf_dev) {
  PH_REQUIRE(m, "ph_model_set_clock_probe: null model");
  m->clock_probe = static_cast<unsigned long long*>(buf_dev);
  return PH_OK;
}

int ph_model_read_slot(ph_model* m, int32_t slot, float* out_dev, int64_t out_numel, void* stream) {
  PH_REQUIRE(m && out_dev && m->last_ws, "ph_model_read_slot: no forward has run");
  PH_REQUIRE(slot >= 0 && slot < m->n_slots && m->last_plan.slots[slot].offset >= 0, "bad slot %d", slot);
  PH_REQUIRE(!m->last_plan.recycle, "activations are recycled in this plan: set the handle option workspace_reuse to 0 (or 2) before the forward to read a slot back");
  const SlotShape& s = m->last_plan.slots[slot];
  PH_REQUIRE(out_numel == (int64_t)m->last_batch * s.c * s.h * s.w, "slot %d has %d x %d x %d x %d elements", slot, m->last_batch, s.c, s.h, s.w);
  if (m->last_plan.fmt != FMT_F32)
    return launch_slot_to_nchw_fmt(m->last_plan.fmt, m->last_ws + s.offset, out_dev, m->last_batch, s.h * s.w, s.cp, s.c, static_cast<hipStream_t>(stream));
  return launch_nhwc_to_nchw(reinterpret_cast<float*>(m->last_ws + s.offset), out_dev, m->last_batch, s.h * s.w, s.cp, s.c,
                             static_cast<hipStream_t>(stream));
}

}  // extern "C"
