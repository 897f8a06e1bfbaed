// Weight forms of the network runtime handle: the host packers that lay the canonical parameters out for each kernel (with the gather maps ph_model_set_params rebuilds
// them through), the table of the forms derived on the device from a packed buffer (derive / refresh: the only code that allocates / re-launches one), and ph_model_create,
// which walks the program once and gives every op its forms (one forms_<kind> routine per op kind over one PackCtx, as forward.hip's fwd_<kind> over ForwardCtx).
#include <algorithm>
#include <map>
#include <type_traits>
#include <vector>

#include "model_internal.h"
#include "train_kernels.h"

#define PH_TRY(expr)               \
  do {                             \
    const int _rc = (expr);        \
    if (_rc != PH_OK) return _rc;  \
  } while (0)

namespace ph {
namespace {

int upload(ph_model* m, const std::vector<float>& host, float** dev) {
  void* p = nullptr;
  PH_HIP_CHECK(hipMalloc(&p, std::max<size_t>(host.size(), 4) * sizeof(float)));
  m->allocs.push_back(p);
  if (host.size() < 4) PH_HIP_CHECK(hipMemset(p, 0, 4 * sizeof(float)));  // (the allocation is rounded up to four elements: its tail holds zeros, not what the memory held before)
  PH_HIP_CHECK(hipMemcpy(p, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice));
  *dev = static_cast<float*>(p);
  return PH_OK;
}

int upload_ints(ph_model* m, const std::vector<int>& host, int** dev) {
  void* p = nullptr;
  PH_HIP_CHECK(hipMalloc(&p, std::max<size_t>(host.size(), 4) * sizeof(int)));
  m->allocs.push_back(p);
  if (host.size() < 4) PH_HIP_CHECK(hipMemset(p, 0, 4 * sizeof(int)));
  PH_HIP_CHECK(hipMemcpy(p, host.data(), host.size() * sizeof(int), hipMemcpyHostToDevice));
  *dev = static_cast<int*>(p);
  return PH_OK;
}

// Upload a packed value array together with its gather map.  `packed_idx` is the SAME packing
// applied to an array holding (canonical index + 1) as doubles (exact for any arena size).
int upload_packed(ph_model* m, const std::vector<float>& packed_val, const std::vector<double>& packed_idx, float** dev) {
  PH_TRY(upload(m, packed_val, dev));
  std::vector<int> map(packed_idx.size());
  for (size_t i = 0; i < packed_idx.size(); ++i) map[i] = (int)((int64_t)packed_idx[i] - 1);
  PackedBuffer pb;
  pb.dst = *dev;
  pb.n = packed_val.size();
  PH_TRY(upload_ints(m, map, &pb.map));
  m->packed.push_back(pb);
  return PH_OK;
}

// Run one packing routine twice -- on the weight values and on their canonical indices -- and upload both.
template <typename PackFn>
int pack_upload(ph_model* m, PackFn&& pack, const float* values, const std::vector<double>& indices, float** dev) {
  std::vector<float> v;
  std::vector<double> x;
  pack(values, v);
  pack(indices.data(), x);
  return upload_packed(m, v, x, dev);
}

int upload_zeros(ph_model* m, size_t n, float** dev) { return upload(m, std::vector<float>(n, 0.f), dev); }  // (not a parameter: nothing in the arena maps onto it)

// ---- host packers: each takes the canonical layout and is run on values (float) and on indices (double) alike

// zero-padded copy of a per-channel vector (bias, LayerNorm affine, layer scale)
auto pad_vec(size_t padded, int n) {
  return [padded, n](const auto* src, auto& out) {
    out.assign(padded, 0);
    for (int k = 0; k < n; ++k) out[k] = src[k];
  };
}

// OIHW (cout, cin_total, 3, 3) -> the conv weight of the data gradient wrt channels
// [ci_off, ci_off + cin_part): Wd[o = ci][i = co][ky][kx] = W[co][ci_off + ci][2-ky][2-kx].
template <typename T>
void dgrad_weight(const T* w, int cout, int cin_total, int ci_off, int cin_part, std::vector<T>& out, int k = 3) {
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
void pack_conv(const T* w, bool transposed, int cin0, int cin1, int cout, int bn, std::vector<T>& out) {
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
template <typename T>
void repack_dma(const std::vector<T>& in, int bn, std::vector<T>& out) {
  out.resize(in.size());
  const size_t panel = (size_t)9 * bn * 16;
  for (size_t base = 0; base < in.size(); base += panel)
    for (int row = 0; row < 9 * bn; ++row)
      for (int k = 0; k < 16; ++k) {
        const int piece = row >> 4, r = row & 15, q = k >> 2, e = k & 3;
        out[base + (size_t)piece * 256 + q * 64 + r * 4 + e] = in[base + (size_t)row * 16 + k];
      }
}

// [tap][ci 16][co 16] (zero padded) from OIHW, for conv3x3_c16_kernel
template <typename T>
void pack_c16(const T* w, int cout, int cin, std::vector<T>& out) {
  out.assign(9 * 256, T(0));
  for (int co = 0; co < cout; ++co)
    for (int ci = 0; ci < cin; ++ci)
      for (int tap = 0; tap < 9; ++tap) out[(size_t)(tap * 16 + ci) * 16 + co] = w[((size_t)co * cin + ci) * 9 + tap];
}

// Row-GEMM weights (gemm_mfma_dma_kernel): Linear (cout, cin) [taps = 1], Conv2d k2 s2 (cout, cin, 2, 2)
// [taps = 4] or Conv2d 3x3 over concat(cin0, cin1) (cout, cin0 + cin1, 3, 3) [taps = 9] ->
// [n_tile][stage][piece = n / 8][slot][row n % 8][4]; a stage is 32 channels of one source at one tap,
// stage order = source, 32-channel slice, tap (taps innermost); slot = channel quad ^ (piece & 1)
// (the LDS image the kernel's DMA writes); zero-padded channels / rows.
template <typename T>
void pack_gemm(const T* w, int cout, int cin0, int cin1, int taps, int bn, std::vector<T>& out) {
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

// CNBlock MLP, first Linear (4C, C) -> [hidden block hb][piece q: C / 8][lane (i = lane & 31, h = lane >> 5)][t]: W1[hb 32 + i][h C / 2 + 4 q + t]
// (the A operand of K step s = 4 q + t of cnblock_mlp_kernel's first product: channels (s, C / 2 + s) in the two lane halves)
template <typename T>
void pack_mlp_w1(const T* w, int c, std::vector<T>& out) {
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
void pack_mlp_w2(const T* w, int c, std::vector<T>& out) {
  const int nhb = 4 * c / 32, nb_ = c / 32;
  out.assign((size_t)nhb * nb_ * 4 * 256, T(0));
  for (int hb = 0; hb < nhb; ++hb)
    for (int nb = 0; nb < nb_; ++nb)
      for (int g = 0; g < 4; ++g)
        for (int lane = 0; lane < 64; ++lane)
          for (int t = 0; t < 4; ++t)
            out[((((size_t)hb * nb_ + nb) * 4 + g) * 64 + lane) * 4 + t] = w[(size_t)(nb * 32 + (lane & 31)) * (4 * c) + hb * 32 + 8 * g + 4 * (lane >> 5) + t];
}

int choose_bn(int coutp) { return coutp >= 64 ? 64 : 32; }
int chunks16(int cin_a, int cin_b) { return pad16(cin_a) / 16 + (cin_b > 0 ? pad16(cin_b) / 16 : 0); }  // 16-channel chunks of a conv's (concatenated) input
size_t n_padded(int coutp, int bn) { return (size_t)((coutp + bn - 1) / bn) * bn; }                       // a bias padded to whole N tiles

// ---- derived forms: buffers computed on the device from a packed buffer (linear combinations of taps, fp16 images: not gathers of parameters).  One entry per kind:
// its size, its launcher -- with the meaning of DerivedBuffer::p[] written beside the call that consumes it -- and who reads it, i.e. when ph_model_set_params may leave
// it stale.  No code outside this table chooses a launcher or an argument order by kind.
struct DerivedForm {
  int64_t (*bytes)(const int* p);
  int (*launch)(const float* src, float* dst, const int* p, hipStream_t s);
  RefreshClass cls;
};

const DerivedForm FORMS[DERIVED_KINDS] = {
    // DERIVED_WINO: Winograd F(2,3) transform.  p = {16-channel panels of the source (N tiles x chunks), N tile of the source (32 or 64)}; refresh_batched hands p[1] to the multi-buffer launch as the segment's N tile
    {[](const int* p) { return wino_pack_floats(p[0], p[1]) * 4; }, [](const float* src, float* dst, const int* p, hipStream_t s) { return launch_wino_pack(src, dst, p[0], p[1], s); },
     REFRESH_BATCHED},
    // DERIVED_F16_PACK: fp16 weight pack of the LDS-DMA panels.  p = {N tiles, chunks of source 0, chunks of source 1, N tile, 1 = plain fp16 | 0 = split (hi, lo)}
    {[](const int* p) { return f16_weight_pack_floats(p[0], p[1], p[2], p[3], p[4]) * 4; },
     [](const float* src, float* dst, const int* p, hipStream_t s) { return launch_f16_weight_pack(src, dst, p[0], p[1], p[2], p[3], p[4], s); }, REFRESH_ALWAYS},
    // DERIVED_WINO2D: F(2x2,3x3) transform of an N-tile-64 packing.  p = {panels, 64}; batched like F(2,3)
    {[](const int* p) { return wino2d_pack_floats(p[0], p[1]) * 4; }, [](const float* src, float* dst, const int* p, hipStream_t s) { return launch_wino2d_pack(src, dst, p[0], p[1], s); },
     REFRESH_BATCHED},
    // DERIVED_W16: wave-private F(2x2,3x3) transform.  p = {16-channel chunks (both sources), N blocks of 16 output channels (1 or 2)}
    {[](const int* p) { return w16_pack_floats(p[0], p[1]) * 4; }, [](const float* src, float* dst, const int* p, hipStream_t s) { return launch_w16_pack(src, dst, p[0], p[1], s); },
     REFRESH_ALWAYS},
    // DERIVED_STEM_WINO2D: F(2x2,3x3) transform of the fused stem's second conv ([position 16][co 16][ci 16]).  No parameters
    {[](const int*) { return (int64_t)16 * 256 * 4; }, [](const float* src, float* dst, const int*, hipStream_t s) { return launch_stem_wino2d_pack(src, dst, s); }, REFRESH_ALWAYS},
    // DERIVED_WINO4: F(4x4,3x3) transform of an N-tile-64 packing.  p = {padded output channels, 16-channel chunks}
    {[](const int* p) { return wino4_pack_floats((p[0] + 63) / 64, p[1]) * 4; }, [](const float* src, float* dst, const int* p, hipStream_t s) { return launch_wino4_pack(src, dst, p[0], p[1], s); },
     REFRESH_INFERENCE},
    // DERIVED_SMALLMAP: small-map F(2x2,3x3) transform.  p = {N blocks of 16 output channels, 16-channel chunks, N tile of the source packing}
    {[](const int* p) { return sm_pack_floats(p[0], p[1]) * 4; }, [](const float* src, float* dst, const int* p, hipStream_t s) { return launch_sm_pack(src, dst, p[0], p[1], p[2], s); },
     REFRESH_INFERENCE},
    // DERIVED_GEMM_F16_IMAGE: fp16 row-GEMM weight image of a Linear / 2x2-stride-2 conv.  p = {cout, cin, taps (1 or 4), N tile of the source packing}
    {[](const int* p) { return gemm_f16_weight_image_halves(fmt_cpad(FMT_F16, p[0]), fmt_cpad(FMT_F16, p[1]), p[2]) * 2; },
     [](const float* src, float* dst, const int* p, hipStream_t s) { return launch_gemm_f16_weight_image(src, dst, p[0], p[1], fmt_cpad(FMT_F16, p[0]), fmt_cpad(FMT_F16, p[1]), p[2], p[3], s); },
     REFRESH_F16_GEMM},
    // DERIVED_STEM_WINO: F(2,3) transform of the fused stem's second conv (12 x [co 16][ci 16]).  No parameters
    {[](const int*) { return (int64_t)12 * 256 * 4; }, [](const float* src, float* dst, const int*, hipStream_t s) { return launch_stem_wino_pack(src, dst, s); }, REFRESH_ALWAYS},
};

struct FormParams {
  int p[5];
};

// Allocate one derived form, compute it (ph_model_create: on the null stream) and note it for refresh(): the only code that allocates one.
int derive(ph_model* m, DerivedKind kind, const float* src, FormParams params, float** dst, hipStream_t s = nullptr) {
  DerivedBuffer db;
  db.kind = kind;
  db.src = src;
  std::copy(params.p, params.p + 5, db.p);
  void* w = nullptr;
  PH_HIP_CHECK(hipMalloc(&w, (size_t)FORMS[kind].bytes(db.p)));
  m->allocs.push_back(w);
  db.dst = static_cast<float*>(w);
  PH_TRY(FORMS[kind].launch(src, db.dst, db.p, s));
  m->derived.push_back(db);
  *dst = db.dst;
  return PH_OK;
}

// Recompute one derived form from its source: the only code that re-launches one.
int refresh(const DerivedBuffer& db, hipStream_t s) { return FORMS[db.kind].launch(db.src, db.dst, db.p, s); }

// Does this handle, with its options as they stand, read the forms of `kind` in `plan` -- or, with no forward at hand (plan == nullptr: ph_model_set_params), may its
// options lead to a plan that does?  ph_model_set_params skips a form this denies and sets the class's stale flag; refresh_stale_weights brings a stale class up to date
// before the first forward for which this holds.  (Truth table: DESIGN.md, the paragraph on ph_model_set_params.)
bool reads_forms(const ph_model* m, DerivedKind kind, const Plan* plan) {
  switch (FORMS[kind].cls) {
    case REFRESH_INFERENCE: {  // (conv_wino4 / conv_smallmap 1: inference plans only; >= 2: every plan)
      const int option = kind == DERIVED_WINO4 ? m->conv_wino4 : m->conv_smallmap;
      return option >= 2 || (plan ? option == 1 && plan->reuse : m->workspace_reuse != 0);
    }
    case REFRESH_F16_GEMM:  // (only a Linear program on its fp16 pipe: plain fp16 with convnext_f16 / swint_f16 -- and a program that has such a form)
      return plan ? plan->fmt == FMT_F16 : (m->conv_precision == 2 && (m->convnext_f16 || m->swint_f16));
    default:
      return true;
  }
}

// One table-driven launch each for the F(2,3) [0] and the F(2x2,3x3) [1] forms (most of a UNet's derived buffers); the tables are built at the first call.
int refresh_batched(ph_model* m, hipStream_t s) {
  static const DerivedKind kinds[2] = {DERIVED_WINO, DERIVED_WINO2D};
  for (int t = 0; t < 2 && !m->pack_tables_built; ++t) {
    std::vector<PackSegment> seg;
    unsigned blocks = 0;
    for (const DerivedBuffer& db : m->derived) {
      if (db.kind != kinds[t]) continue;
      const unsigned long long total = (unsigned long long)FORMS[db.kind].bytes(db.p) / 4;
      if (total == 0) continue;
      seg.push_back(PackSegment{db.src, db.dst, total, db.p[1], blocks});
      blocks += (unsigned)((total + 1023) / 1024);
    }
    void* table = nullptr;
    if (!seg.empty()) {
      PH_HIP_CHECK(hipMalloc(&table, seg.size() * sizeof(PackSegment)));
      m->allocs.push_back(table);
      PH_HIP_CHECK(hipMemcpy(table, seg.data(), seg.size() * sizeof(PackSegment), hipMemcpyHostToDevice));
    }
    m->pack_table_dev[t] = table;
    m->pack_segments[t] = (int)seg.size();
    m->pack_blocks[t] = blocks;
  }
  m->pack_tables_built = true;
  PH_TRY(launch_wino_pack_multi(static_cast<const PackSegment*>(m->pack_table_dev[0]), m->pack_segments[0], m->pack_blocks[0], s));
  return launch_wino2d_pack_multi(static_cast<const PackSegment*>(m->pack_table_dev[1]), m->pack_segments[1], m->pack_blocks[1], s);
}

}  // namespace

// The derived-form half of ph_model_set_params (the packed buffers have just been gathered from `params_flat_dev` on `s`).
int refresh_derived(ph_model* m, const float* params_flat_dev, hipStream_t s) {
  PH_TRY(refresh_batched(m, s));
  for (const DerivedBuffer& db : m->derived) {
    const RefreshClass cls = FORMS[db.kind].cls;
    if (cls == REFRESH_BATCHED) continue;  // in the two launches above
    if (!reads_forms(m, db.kind, nullptr)) {  // a training step does not pay for a form only other plans read: the next forward that wants it refreshes it (refresh_stale_weights)
      m->forms_stale[cls] = true;
      continue;
    }
    PH_TRY(refresh(db, s));
  }
  // fused GRN plan ("grn_fuse"): the constant term W2 grn.bias + b2 of a residual Linear behind a GRN op follows the parameters.  Only a program whose first Linear
  // carries the GELU can take that plan (fuses_grn), so an unfused (training) program never pays for this
  for (size_t i = 2; i < m->ops.size(); ++i) {
    const PackedOp& op = m->ops[i];
    const ph_op_desc& g = m->ops[i - 1].d;
    const ph_op_desc& l1 = m->ops[i - 2].d;
    if (!op.b_grn_dev || g.kind != PH_OP_GRN || !(l1.kind == PH_OP_LINEAR && l1.flags == PH_FLAG_GELU)) continue;
    PH_TRY(launch_grn_fold_bias(params_flat_dev + m->weight_offset[op.d.weight], params_flat_dev + m->weight_offset[op.d.bias], params_flat_dev + m->weight_offset[g.bias], op.b_grn_dev,
                                op.d.cout, op.d.cin0, s));
  }
  return PH_OK;
}

// The forms ph_model_set_params left stale: a class is derived again, whole, before the first forward that reads one of its kinds.
int refresh_stale_weights(ph_model* m, const Plan& plan, hipStream_t s) {
  for (int cls = 0; cls < REFRESH_CLASSES; ++cls) {
    if (!m->forms_stale[cls]) continue;
    bool read = false;
    for (int kind = 0; kind < DERIVED_KINDS; ++kind) read = read || (FORMS[kind].cls == cls && reads_forms(m, (DerivedKind)kind, &plan));
    if (!read) continue;
    for (const DerivedBuffer& db : m->derived)
      if (FORMS[db.kind].cls == cls) PH_TRY(refresh(db, s));
    m->forms_stale[cls] = false;
  }
  return PH_OK;
}

// fp16 weight packs of every 3x3 conv / transposed conv, derived on the device from the fp32 LDS-DMA panels the first time a
// forward needs them (and again after every ph_model_set_params, through m->derived).  Allocates: not capturable -- a
// hipGraph user runs one eager forward first (HipBackend does).
int ensure_f16_weights(ph_model* m, int plain, hipStream_t s) {
  for (PackedOp& op : m->ops) {
    const ph_op_desc& d = op.d;
    if ((d.kind != PH_OP_CONV && d.kind != PH_OP_CONVT) || op.w_f16_dev[plain]) continue;
    PH_REQUIRE(op.w_dma_dev && (op.bn == 32 || op.bn == 64), "conv op has no LDS-DMA weight panels");
    PH_TRY(derive(m, DERIVED_F16_PACK, op.w_dma_dev, {{(pad16(d.cout) + op.bn - 1) / op.bn, pad16(d.cin0) / 16, d.cin1 > 0 ? pad16(d.cin1) / 16 : 0, op.bn, plain}}, &op.w_f16_dev[plain], s));
  }
  return PH_OK;
}

namespace {

// ---- ph_model_create: what the per-op routines share
struct PackCtx {
  ph_model* const m;
  const ph_op_desc* const ops;
  const int n_ops;
  const float* const* const weights;
  const int64_t* const weight_numel;
  const int n_weights, n_outputs;
  int i = 0;              // index of the op being packed
  bool reported = false;  // fail() has worded this op's error
  std::map<int, std::vector<double>> index;  // index_array() of the current op's parameters

  bool widx_ok(int k) const { return k >= 0 && k < n_weights; }
  int fail(const char* msg) {
    set_error("ph_model_create: op %d: %s", i, msg);
    reported = true;
    return PH_E_INVALID;
  }
  // (canonical arena index + 1) of every element of weights[wi]: what a packer runs on to give the gather map
  const std::vector<double>& index_array(int wi) {
    auto it = index.find(wi);
    if (it != index.end()) return it->second;
    std::vector<double>& v = index[wi];
    v.resize((size_t)(wi >= 0 ? weight_numel[wi] : 0));
    for (size_t k = 0; k < v.size(); ++k) v[k] = (double)(m->weight_offset[wi] + (int64_t)k + 1);
    return v;
  }
  template <typename PackFn>
  int pack(PackFn&& fn, int wi, float** dev) {
    return pack_upload(m, fn, weights[wi], index_array(wi), dev);
  }
  bool has_weight_and_bias(const ph_op_desc& d) const { return widx_ok(d.weight) && widx_ok(d.bias); }
};

int forms_scale_add(PackCtx& c, PackedOp& op) {
  const ph_op_desc& d = op.d;
  if (!c.widx_ok(d.weight) || c.weight_numel[d.weight] != d.cout || d.cin0 != d.cout || d.src1 < 0) return c.fail("scale-add needs a (C) scale and two sources");
  return c.pack(pad_vec(pad16(d.cout), d.cout), d.weight, &op.w_dev);
}

int forms_stem(PackCtx& c, PackedOp& op) {
  const ph_op_desc& d = op.d;
  if (d.ksize != 3 || d.cmid < 1 || d.cmid > 16 || d.cout < 1 || d.cout > 16 || (d.cin0 != 1 && d.cin0 != 3)) return c.fail("fused stem needs kernel 3, 1 or 3 input channels and <= 16 filters");
  if (!c.widx_ok(d.weight) || !c.widx_ok(d.bias) || !c.widx_ok(d.weight2) || !c.widx_ok(d.bias2)) return c.fail("weight index out of range");
  if (c.weight_numel[d.weight] != (int64_t)d.cmid * d.cin0 * 9 || c.weight_numel[d.bias] != d.cmid || c.weight_numel[d.weight2] != (int64_t)d.cout * d.cmid * 9 ||
      c.weight_numel[d.bias2] != d.cout)
    return c.fail("stem weight size mismatch");
  auto pack_w0 = [&](const auto* w0, auto& p0) {  // [tap][ci][co 16]
    p0.assign((size_t)9 * d.cin0 * 16, 0);
    for (int co = 0; co < d.cmid; ++co)
      for (int ci = 0; ci < d.cin0; ++ci)
        for (int tap = 0; tap < 9; ++tap) p0[((size_t)tap * d.cin0 + ci) * 16 + co] = w0[((size_t)co * d.cin0 + ci) * 9 + tap];
  };
  auto pack_w1 = [&](const auto* w1, auto& p1) {  // [tap][co 16][ci 16]
    p1.assign((size_t)9 * 16 * 16, 0);
    for (int co = 0; co < d.cout; ++co)
      for (int ci = 0; ci < d.cmid; ++ci)
        for (int tap = 0; tap < 9; ++tap) p1[((size_t)tap * 16 + co) * 16 + ci] = w1[((size_t)co * d.cmid + ci) * 9 + tap];
  };
  PH_TRY(c.pack(pack_w0, d.weight, &op.w_dev));
  PH_TRY(c.pack(pad_vec(16, d.cmid), d.bias, &op.b_dev));
  PH_TRY(c.pack(pack_w1, d.weight2, &op.w2_dev));
  PH_TRY(c.pack(pad_vec(16, d.cout), d.bias2, &op.b2_dev));
  PH_TRY(derive(c.m, DERIVED_STEM_WINO, op.w2_dev, {}, &op.w_wino_dev));  // Winograd form of the second conv ...
  return derive(c.m, DERIVED_STEM_WINO2D, op.w2_dev, {}, &op.w_stem2_dev);  // ... and its F(2x2,3x3) form (the default)
}

// k x k "same" conv, k = 1, 5, 7, 9 (and the 7x7 convs of a stem block), as a k^2-tap row GEMM (mode 5)
int forms_conv_kxk(PackCtx& c, PackedOp& op) {
  const ph_op_desc& d = op.d;
  if (!(d.ksize & 1) || d.ksize < 1 || d.ksize > 9) return c.fail("kernel_size must be odd and <= 9");
  if (c.weight_numel[d.weight] != (int64_t)(d.cin0 + d.cin1) * d.cout * d.ksize * d.ksize) return c.fail("weight size mismatch");
  const int coutp = pad16(d.cout), taps = d.ksize * d.ksize;
  op.bn_g = gemm_choose_bn(coutp);
  PH_TRY(c.pack([&](const auto* w, auto& out) { pack_gemm(w, d.cout, d.cin0, d.cin1, taps, op.bn_g, out); }, d.weight, &op.w_gemm_dev));
  PH_TRY(c.pack(pad_vec(n_padded(coutp, op.bn_g), d.cout), d.bias, &op.b_gemm_dev));
  if (d.kind != PH_OP_CONV) return PH_OK;
  // data-gradient weights (training): the same k x k row GEMM on the flipped, in/out-swapped taps, one per concat source
  const int cin_total = d.cin0 + d.cin1;
  const int parts[2] = {d.cin0, d.cin1}, offs[2] = {0, d.cin0};
  int max_bn = 32;
  for (int part = 0; part < 2; ++part) {
    if (parts[part] <= 0) continue;
    op.bn_dk[part] = gemm_choose_bn(pad16(parts[part]));
    max_bn = std::max(max_bn, op.bn_dk[part]);
    auto pack_dk = [&](const auto* w, auto& out) {
      std::remove_reference_t<decltype(out)> dw;
      dgrad_weight(w, d.cout, cin_total, offs[part], parts[part], dw, d.ksize);
      pack_gemm(dw.data(), parts[part], d.cout, 0, taps, op.bn_dk[part], out);
    };
    PH_TRY(c.pack(pack_dk, d.weight, &op.wdk_gemm_dev[part]));
  }
  return upload_zeros(c.m, (size_t)pad16(std::max(d.cin0, d.cin1)) + 2 * max_bn, &op.zero_bias_dev);
}

// The Winograd forms of one [n_tile][chunk][tap][bn][16] packing `src` of a 3x3 conv (cin_a + cin_b -> cout_, N tile bn): F(2,3) (N tile 32 or 64) and F(2x2,3x3)
// (conv3x3_wino2d_kernel, N tile 64), then -- `tail` -- the wave-private F(2x2,3x3) form (conv3x3_w16_kernel: N tile 32, the channel counts of w16_shape_ok) and
// F(4x4,3x3) (conv3x3_wino4_kernel: N tile 64, derived from 64 padded input channels on -- 4x the direct weights' bytes; which layers take the kernel is
// conv_wino4_min_cin + the time model).  The forward conv's and the data-gradient convs'.
// (the parameters of each form, FormParams as FORMS[] reads them, and whether the form exists for that packing: shared with ph_debug_conv3x3_run)
bool wino_form(int cin_a, int cin_b, int cout_, int bn, FormParams& p) {
  if (bn != 64 && bn != 32) return false;
  p = {{((pad16(cout_) + bn - 1) / bn) * chunks16(cin_a, cin_b), bn}};
  return true;
}
bool wino2_form(int cin_a, int cin_b, int cout_, int bn, FormParams& p) {
  if (bn != 64) return false;
  p = {{((pad16(cout_) + 63) / 64) * chunks16(cin_a, cin_b), 64}};
  return true;
}
bool wino4_form(int cin_a, int cin_b, int cout_, int bn, FormParams& p) {
  if (bn != 64 || 16 * chunks16(cin_a, cin_b) < 64) return false;
  p = {{pad16(cout_), chunks16(cin_a, cin_b)}};
  return true;
}
bool w16_form(int cin_a, int cin_b, int cout_, int bn, FormParams& p) {
  const int cip = pad16(cin_a), cibp = cin_b > 0 ? pad16(cin_b) : 0, cop = pad16(cout_);
  if (bn != 32 || !w16_shape_ok(cip, cibp, cop)) return false;
  p = {{(cip + cibp) / 16, cop / 16}};
  return true;
}
FormParams sm_form(int cin_a, int cin_b, int cout_, int bn) { return {{pad16(cout_) / 16, chunks16(cin_a, cin_b), bn}}; }  // (every 3x3 conv has it)
// 32 output channels, K >= 64: the layer also gets a packing with an N tile of 64 (rows 32 .. 63 zero) for the half-empty-tile form of the F(2x2,3x3) / F(4x4,3x3) kernels
bool has_n64_form(int cin_a, int cin_b, int cout_, int bn) { return bn == 32 && pad16(cout_) == 32 && 16 * chunks16(cin_a, cin_b) >= 64; }

int derive_wino(PackCtx& c, const float* src, int cin_a, int cin_b, int cout_, int bn, float** dst) {
  FormParams p;
  return wino_form(cin_a, cin_b, cout_, bn, p) ? derive(c.m, DERIVED_WINO, src, p, dst) : PH_OK;
}
int derive_wino2(PackCtx& c, const float* src, int cin_a, int cin_b, int cout_, int bn, float** dst) {
  FormParams p;
  return wino2_form(cin_a, cin_b, cout_, bn, p) ? derive(c.m, DERIVED_WINO2D, src, p, dst) : PH_OK;
}
int derive_wino4(PackCtx& c, const float* src, int cin_a, int cin_b, int cout_, int bn, float** dst) {
  FormParams p;
  return wino4_form(cin_a, cin_b, cout_, bn, p) ? derive(c.m, DERIVED_WINO4, src, p, dst) : PH_OK;
}
int derive_w16(PackCtx& c, const float* src, int cin_a, int cin_b, int cout_, int bn, float** dst) {
  FormParams p;
  return w16_form(cin_a, cin_b, cout_, bn, p) ? derive(c.m, DERIVED_W16, src, p, dst) : PH_OK;
}

// 3x3 conv (not transposed): the forms of the forward
int forms_conv3x3_forward(PackCtx& c, PackedOp& op) {
  const ph_op_desc& d = op.d;
  const int coutp = pad16(d.cout);
  PH_TRY(derive_wino(c, op.w_dev, d.cin0, d.cin1, d.cout, op.bn, &op.w_wino_dev));
  PH_TRY(derive_wino2(c, op.w_dev, d.cin0, d.cin1, d.cout, op.bn, &op.w_wino2_dev));
  if (has_n64_form(d.cin0, d.cin1, d.cout, op.bn)) {
    // 32 output channels, K >= 64: a second packing with an N tile of 64 (rows 32 .. 63 zero) for the F(2x2,3x3) kernel's half-empty-tile form (conv_n32_wino2d)
    PH_TRY(c.pack([&](const auto* w, auto& out) { pack_conv(w, false, d.cin0, d.cin1, d.cout, 64, out); }, d.weight, &op.w_n64_dev));
    PH_TRY(c.pack(pad_vec(64, d.cout), d.bias, &op.b_n64_dev));
    PH_TRY(derive_wino2(c, op.w_n64_dev, d.cin0, d.cin1, d.cout, 64, &op.w_wino2_dev));
  }
  PH_TRY(derive_wino4(c, op.w_dev, d.cin0, d.cin1, d.cout, op.bn, &op.w_wino4_dev));
  if (op.w_n64_dev) PH_TRY(derive_wino4(c, op.w_n64_dev, d.cin0, d.cin1, d.cout, 64, &op.w_wino4_dev));  // (Cout 32, K >= 64: the kernel's waves of the empty N half skip their MFMAs)
  PH_TRY(derive_w16(c, op.w_dev, d.cin0, d.cin1, d.cout, op.bn, &op.w_w16_dev));
  // small-map F(2x2,3x3) weights (conv3x3_sm_kernel): 16/9 of the direct weights' bytes, every 3x3 conv
  PH_TRY(derive(c.m, DERIVED_SMALLMAP, op.w_dev, sm_form(d.cin0, d.cin1, d.cout, op.bn), &op.w_sm_dev));
  // row-GEMM form for feature maps too small for the 16x32-pixel tiles
  op.bn_g = gemm_choose_bn(coutp);
  PH_TRY(c.pack([&](const auto* w, auto& out) { pack_gemm(w, d.cout, d.cin0, d.cin1, 9, op.bn_g, out); }, d.weight, &op.w_gemm_dev));
  return c.pack(pad_vec(n_padded(coutp, op.bn_g), d.cout), d.bias, &op.b_gemm_dev);
}

// 16 -> 16 channel 3x3 conv: conv3x3_c16_kernel's weights and those of its data gradient
int forms_conv_c16(PackCtx& c, PackedOp& op) {
  const ph_op_desc& d = op.d;
  auto pack_16d = [&](const auto* w, auto& out) {
    std::remove_reference_t<decltype(out)> dw;
    dgrad_weight(w, d.cout, d.cin0, 0, d.cin0, dw);
    pack_c16(dw.data(), d.cin0, d.cout, out);
  };
  PH_TRY(c.pack([&](const auto* w, auto& out) { pack_c16(w, d.cout, d.cin0, out); }, d.weight, &op.w16_dev));
  return c.pack(pack_16d, d.weight, &op.wd16_dev);
}

// ConvTranspose2d(k3, s2, p1, op1): output (oy, ox) = (2y - 1 + ky, 2x - 1 + kx).  Even output rows see only ky = 1
// (input row y), odd rows ky = 0 (input row y + 1) and ky = 2 (row y) -- likewise in x: four output phases with
// 1, 2, 2, 4 taps.  Each phase is one row GEMM over the input grid (mode 3) whose tap t reads input pixel
// (y + dy, x + dx); weights per phase: wp[co][ci][t] = Wt[ci][co][ky(t)][kx(t)].  Then the folded BatchNorm and the data gradient (mode 4).
template <typename T>
void pack_convt_phase(const T* w, int cout, int cin, int ph, int bn, std::vector<T>& out) {  // the row-GEMM pack of output phase ph = 2 py + px from the IOHW (cin, cout, 3, 3) weight
  const int py = ph >> 1, px = ph & 1, nt = (1 + py) * (1 + px);
  std::vector<T> wp((size_t)cout * cin * nt);
  for (int t = 0; t < nt; ++t) {
    const int ty = px ? t >> 1 : t, tx = px ? t & 1 : 0;
    const int ky = py ? 2 * ty : 1, kx = px ? 2 * tx : 1;  // tap t reads (y + 1 - ty, x + 1 - tx): ky = 0 <-> dy = 1
    for (int co = 0; co < cout; ++co)
      for (int ci = 0; ci < cin; ++ci) wp[((size_t)co * cin + ci) * nt + t] = w[(((size_t)ci * cout + co) * 3 + ky) * 3 + kx];
  }
  pack_gemm(wp.data(), cout, cin, 0, nt, bn, out);
}

int forms_convt_phases(PackCtx& c, PackedOp& op) {
  const ph_op_desc& d = op.d;
  const int coutp = pad16(d.cout);
  op.bn_t = gemm_choose_bn(coutp);
  const size_t npad_t = n_padded(coutp, op.bn_t);
  for (int ph = 0; ph < 4; ++ph)
    PH_TRY(c.pack([&](const auto* w, auto& out) { pack_convt_phase(w, d.cout, d.cin0, ph, op.bn_t, out); }, d.weight, &op.wt_phase_dev[ph]));
  PH_TRY(c.pack(pad_vec(npad_t, d.cout), d.bias, &op.bt_dev));
  if (d.weight2 >= 0) {  // folded BatchNorm (eval): y = act(scale * (conv + bias) + shift)
    if (!c.widx_ok(d.weight2) || !c.widx_ok(d.bias2) || c.weight_numel[d.weight2] != d.cout || c.weight_numel[d.bias2] != d.cout) return c.fail("transposed conv: scale / shift must be (cout)");
    PH_TRY(c.pack(pad_vec(npad_t, d.cout), d.weight2, &op.wt_scale_dev));
    PH_TRY(c.pack(pad_vec(npad_t, d.cout), d.bias2, &op.wt_shift_dev));
  }
  // data gradient = Conv2d(dY, Wt as (out = cin0, in = cout, 3, 3), stride 2, pad 1): the ConvTranspose2d weight as it lies in memory
  const int cinp = pad16(d.cin0);
  op.bn_td = gemm_choose_bn(cinp);
  PH_TRY(c.pack([&](const auto* w, auto& out) { pack_gemm(w, d.cin0, d.cout, 0, 9, op.bn_td, out); }, d.weight, &op.wt_dgrad_dev));
  return upload_zeros(c.m, (size_t)cinp + 128, &op.zero_bias_dev);
}

// 3x3 conv: data-gradient weights (training; flipped taps, in/out swapped) and their Winograd forms, one set per concat source
int forms_conv3x3_dgrad(PackCtx& c, PackedOp& op) {
  const ph_op_desc& d = op.d;
  const int cin_total = d.cin0 + d.cin1;
  const int parts[2] = {d.cin0, d.cin1}, offs[2] = {0, d.cin0};
  int max_bn = 32;
  for (int part = 0; part < 2; ++part) {
    if (parts[part] <= 0) continue;
    const int bn = op.bn_d[part] = choose_bn(pad16(parts[part]));
    max_bn = std::max(max_bn, bn);
    auto pack_d = [&](const auto* w, auto& out) {
      std::remove_reference_t<decltype(out)> dw;
      dgrad_weight(w, d.cout, cin_total, offs[part], parts[part], dw);
      pack_conv(dw.data(), false, d.cout, 0, parts[part], bn, out);
    };
    auto pack_dd = [&](const auto* w, auto& out) {
      std::remove_reference_t<decltype(out)> tmp;
      pack_d(w, tmp);
      repack_dma(tmp, bn, out);
    };
    PH_TRY(c.pack(pack_d, d.weight, &op.wd_dev[part]));
    PH_TRY(c.pack(pack_dd, d.weight, &op.wd_dma_dev[part]));
    PH_TRY(derive_wino(c, op.wd_dev[part], d.cout, 0, parts[part], bn, &op.wd_wino_dev[part]));
    PH_TRY(derive_wino2(c, op.wd_dev[part], d.cout, 0, parts[part], bn, &op.wd_wino2_dev[part]));
    PH_TRY(derive_w16(c, op.wd_dev[part], d.cout, 0, parts[part], bn, &op.wd_w16_dev[part]));
    PH_TRY(derive_wino4(c, op.wd_dev[part], d.cout, 0, parts[part], bn, &op.wd_wino4_dev[part]));
  }
  return upload_zeros(c.m, (size_t)pad16(std::max(d.cin0, d.cin1)) + max_bn, &op.zero_bias_dev);
}

int forms_conv(PackCtx& c, PackedOp& op) {
  const ph_op_desc& d = op.d;
  const bool tr = d.kind == PH_OP_CONVT;
  if (!c.has_weight_and_bias(d)) return c.fail("weight index out of range");
  if (c.weight_numel[d.bias] != d.cout) return c.fail("bias size mismatch");
  if (tr && d.ksize != 3) return c.fail("transposed conv: only kernel 3 (stride 2, padding 1, output padding 1)");
  if (d.ksize != 3) return forms_conv_kxk(c, op);  // (inference, and the data gradient of a Conv2d)
  if (tr && d.cin1 != 0) return c.fail("transposed conv takes one source");
  if (c.weight_numel[d.weight] != (int64_t)(d.cin0 + d.cin1) * d.cout * 9) return c.fail("weight size mismatch");
  const int coutp = pad16(d.cout);
  op.bn = choose_bn(coutp);
  auto pack_reg = [&](const auto* w, auto& out) { pack_conv(w, tr, d.cin0, d.cin1, d.cout, op.bn, out); };
  auto pack_dma = [&](const auto* w, auto& out) {
    std::remove_reference_t<decltype(out)> tmp;
    pack_reg(w, tmp);
    repack_dma(tmp, op.bn, out);
  };
  PH_TRY(c.pack(pack_reg, d.weight, &op.w_dev));
  PH_TRY(c.pack(pack_dma, d.weight, &op.w_dma_dev));
  PH_TRY(c.pack(pad_vec(n_padded(coutp, op.bn), d.cout), d.bias, &op.b_dev));
  if (!tr) PH_TRY(forms_conv3x3_forward(c, op));
  if (!tr && d.cin1 == 0 && d.cin0 <= 16 && d.cout <= 16) PH_TRY(forms_conv_c16(c, op));
  return tr ? forms_convt_phases(c, op) : forms_conv3x3_dgrad(c, op);
}

// [tap][ci][Cp] from OIHW (cout, cin, k, k); the patch stem (k x k, stride = cmid, padding 1) shares the layout
int forms_input_conv(PackCtx& c, PackedOp& op) {
  const ph_op_desc& d = op.d;
  if (!c.has_weight_and_bias(d)) return c.fail("weight index out of range");
  if (c.weight_numel[d.bias] != d.cout) return c.fail("bias size mismatch");
  if (d.kind == PH_OP_INPUT_CONV && (!(d.ksize & 1) || d.ksize < 1 || d.ksize > 9)) return c.fail("kernel_size must be odd and <= 9");
  if (d.kind == PH_OP_PATCH_STEM && (d.ksize < 2 || d.ksize > 8 || d.cmid < 1 || d.cmid > d.ksize)) return c.fail("patch stem needs 2 <= kernel <= 8 and 1 <= stride <= kernel");
  if (d.kind == PH_OP_PATCH_STEM && (d.flags & PH_FLAG_PAD0_NORM) && (d.cin0 < 1 || d.cin0 > 4)) return c.fail("a padding-0 patch stem with input statistics takes 1..4 input channels");
  const int kk = d.ksize * d.ksize;
  if (c.weight_numel[d.weight] != (int64_t)d.cin0 * d.cout * kk) return c.fail("weight size mismatch");
  const int coutp = pad16(d.cout);
  auto pack_in = [&](const auto* w, auto& out) {
    out.assign((size_t)kk * d.cin0 * coutp, 0);
    for (int co = 0; co < d.cout; ++co)
      for (int ci = 0; ci < d.cin0; ++ci)
        for (int tap = 0; tap < kk; ++tap) out[((size_t)tap * d.cin0 + ci) * coutp + co] = w[((size_t)co * d.cin0 + ci) * kk + tap];
  };
  PH_TRY(c.pack(pack_in, d.weight, &op.w_dev));
  return c.pack(pad_vec(coutp, d.cout), d.bias, &op.b_dev);
}

// 1x1 head weight (cout, cin) -> [co][Cp], zero-padded channels
template <typename T>
void pack_head_w(const T* w, int cout, int cin, std::vector<T>& out) {
  const int cp = pad16(cin);
  out.assign((size_t)cout * cp, T(0));
  for (int co = 0; co < cout; ++co)
    for (int ci = 0; ci < cin; ++ci) out[(size_t)co * cp + ci] = w[(size_t)co * cin + ci];
}

int forms_head(PackCtx& c, PackedOp& op) {
  const ph_op_desc& d = op.d;
  if (!c.has_weight_and_bias(d)) return c.fail("weight index out of range");
  if (c.weight_numel[d.bias] != d.cout) return c.fail("bias size mismatch");
  if (c.weight_numel[d.weight] != (int64_t)d.cin0 * d.cout) return c.fail("weight size mismatch");
  if (d.out_index < 0 || d.out_index >= c.n_outputs) return c.fail("bad out_index");
  PH_TRY(c.pack([&](const auto* w, auto& out) { pack_head_w(w, d.cout, d.cin0, out); }, d.weight, &op.w_dev));
  return c.pack(pad_vec(d.cout, d.cout), d.bias, &op.b_dev);
}

// (C, 1, 7, 7) -> [tap][Cp]
int forms_dwconv(PackCtx& c, PackedOp& op) {
  const ph_op_desc& d = op.d;
  if (!c.has_weight_and_bias(d)) return c.fail("weight index out of range");
  if (d.ksize != 7 || d.cin0 != d.cout) return c.fail("depthwise conv must be 7x7 with cin == cout");
  if (c.weight_numel[d.weight] != (int64_t)d.cout * 49 || c.weight_numel[d.bias] != d.cout) return c.fail("weight size mismatch");
  const int cp = pad16(d.cout);
  auto pack_dw = [&](bool flip) {  // flip: the data gradient = the same kernel on the spatially flipped taps
    return [&d, cp, flip](const auto* w, auto& out) {
      out.assign((size_t)49 * cp, 0);
      for (int ch = 0; ch < d.cout; ++ch)
        for (int tap = 0; tap < 49; ++tap) out[(size_t)(flip ? 48 - tap : tap) * cp + ch] = w[(size_t)ch * 49 + tap];
    };
  };
  PH_TRY(c.pack(pack_dw(false), d.weight, &op.w_dev));
  PH_TRY(c.pack(pad_vec(cp, d.cout), d.bias, &op.b_dev));
  return c.pack(pack_dw(true), d.weight, &op.dw_flip_dev);
}

// LayerNorm, GRN, patch merge: a per-channel weight and bias, padded alike; only what makes the op valid differs
int forms_affine(PackCtx& c, PackedOp& op) {
  const ph_op_desc& d = op.d;
  if (d.kind == PH_OP_PATCH_MERGE && (d.flags & PH_FLAG_NO_NORM)) {  // the gather alone: nothing to pack
    if (d.cout != 4 * d.cin0 || (d.cin0 & 15) || d.src0 < 0 || d.weight >= 0 || d.bias >= 0) return c.fail("a patch merge without a norm needs a channel count that is a multiple of 16 and no parameters");
    return PH_OK;
  }
  if (!c.has_weight_and_bias(d)) return c.fail("weight index out of range");
  const bool sized = c.weight_numel[d.weight] == d.cout && c.weight_numel[d.bias] == d.cout;
  if (d.kind == PH_OP_LAYERNORM && (d.cin0 != d.cout || !sized)) return c.fail("LayerNorm affine size mismatch");
  if (d.kind == PH_OP_LAYERNORM && (d.flags & PH_FLAG_RESIDUAL) && (d.src0 < 0 || d.src1 < 0 || d.src1 == d.dst || d.src0 == d.dst)) return c.fail("a residual LayerNorm needs two sources and a slot of its own");
  if (d.kind == PH_OP_GRN && (d.cin0 != d.cout || d.src0 < 0 || !sized)) return c.fail("GRN needs a (C) weight and bias");
  if (d.kind == PH_OP_PATCH_MERGE && (d.cout != 4 * d.cin0 || (d.cin0 & 15) || !sized)) return c.fail("patch merge needs a channel count that is a multiple of 16 and a (4C) LayerNorm affine");
  const size_t cp = d.kind == PH_OP_PATCH_MERGE ? d.cout : pad16(d.cout);
  PH_TRY(c.pack(pad_vec(cp, d.cout), d.weight, &op.w_dev));
  return c.pack(pad_vec(cp, d.cout), d.bias, &op.b_dev);
}

// weight = relative_position_bias_table ((2w - 1)^2, heads) -> head-major; bias = qkv.bias (3C): the q, k, v of a padded token
int forms_window_attn(PackCtx& c, PackedOp& op) {
  const ph_op_desc& d = op.d;
  if (!c.has_weight_and_bias(d)) return c.fail("weight index out of range");
  const int heads = d.cin1, rel = (2 * d.ksize - 1) * (2 * d.ksize - 1);
  if (d.ksize < 2 || d.ksize > 8) return c.fail("window attention needs 2 <= window_size <= 8");
  if (heads < 1 || d.cout != heads * 32 || d.cin0 != 3 * d.cout) return c.fail("window attention needs head dimension 32 and a (3C) qkv source");
  if (d.cmid < 0 || d.cmid >= d.ksize) return c.fail("window attention shift must be smaller than the window");
  if (c.weight_numel[d.weight] != (int64_t)rel * heads || c.weight_numel[d.bias] != d.cin0) return c.fail("weight size mismatch");
  auto pack_tbl = [&](const auto* w, auto& out) {
    out.assign((size_t)rel * heads, 0);
    for (int r = 0; r < rel; ++r)
      for (int a = 0; a < heads; ++a) out[(size_t)a * rel + r] = w[(size_t)r * heads + a];
  };
  PH_TRY(c.pack(pack_tbl, d.weight, &op.w_dev));
  return c.pack(pad_vec(d.cin0, d.cin0), d.bias, &op.b_dev);
}

// Swinv2's cosine attention.  All three tensors are DERIVED by the host (float64, from logit_scale, the continuous-position-bias MLP and the query / value biases):
// weight = 16 sigmoid(bias table), already head-major (heads, (2w - 1)^2); bias = (3C) query.bias | zeros | value.bias; weight2 = (heads) exp(min(logit_scale, log 100))
int forms_window_attn_v2(PackCtx& c, PackedOp& op) {
  const ph_op_desc& d = op.d;
  if (!c.has_weight_and_bias(d) || !c.widx_ok(d.weight2)) return c.fail("weight index out of range");
  const int heads = d.cin1, rel = (2 * d.ksize - 1) * (2 * d.ksize - 1);
  if (d.ksize < 2 || d.ksize > 24) return c.fail("cosine window attention needs 2 <= window_size <= 24");
  if (heads < 1 || d.cout != heads * 32 || d.cin0 != 3 * d.cout || d.src0 < 0) return c.fail("cosine window attention needs head dimension 32 and a (3C) qkv source");
  if (d.cmid < 0 || d.cmid >= d.ksize) return c.fail("cosine window attention shift must be smaller than the window");
  if (c.weight_numel[d.weight] != (int64_t)rel * heads || c.weight_numel[d.bias] != d.cin0 || c.weight_numel[d.weight2] != heads) return c.fail("weight size mismatch");
  PH_TRY(c.pack(pad_vec((size_t)rel * heads, rel * heads), d.weight, &op.w_dev));
  PH_TRY(c.pack(pad_vec(d.cin0, d.cin0), d.bias, &op.b_dev));
  return c.pack(pad_vec(std::max(heads, 4), heads), d.weight2, &op.w2_dev);
}

// Linear / 2x2-stride-2 conv: data-gradient weights (training): dX = dY * W, one transposed matrix per tap, + a zero bias
int forms_linear_dgrad(PackCtx& c, PackedOp& op, int segs) {
  const ph_op_desc& d = op.d;
  const int cinp = pad16(d.cin0);
  op.bn_dg = gemm_choose_bn(cinp);
  for (int tap = 0; tap < segs; ++tap) {
    auto pack_t = [&](const auto* w, auto& out) {
      std::remove_reference_t<decltype(out)> wt((size_t)d.cin0 * d.cout);
      for (int co = 0; co < d.cout; ++co)
        for (int ci = 0; ci < d.cin0; ++ci) wt[(size_t)ci * d.cout + co] = w[((size_t)co * d.cin0 + ci) * segs + tap];
      pack_gemm(wt.data(), d.cin0, d.cout, 0, 1, op.bn_dg, out);
    };
    PH_TRY(c.pack(pack_t, d.weight, &op.wd_gemm_dev[tap]));
  }
  return upload_zeros(c.m, (size_t)cinp + 128, &op.zero_bias_dev);
}

// Residual Linear behind a GRN op, fused GRN plan: W2 (s x + grn.bias) + b2 = (W2 diag(s)) x + (W2 grn.bias + b2); the second term is constant per set of parameters
// (ph_model_set_params recomputes it on the device, bit for bit this sum: launch_grn_fold_bias)
int forms_grn_bias_fold(PackCtx& c, PackedOp& op, size_t npad) {
  const ph_op_desc& d = op.d;
  const ph_op_desc& g = c.ops[c.i - 1];
  std::vector<float> fb(npad, 0.f);
  const float* w2 = c.weights[d.weight];
  const float* gb = c.weights[g.bias];
  for (int co = 0; co < d.cout; ++co) {
    double acc = c.weights[d.bias][co];
    for (int ci = 0; ci < d.cin0; ++ci) acc += (double)w2[(size_t)co * d.cin0 + ci] * (double)gb[ci];
    fb[co] = (float)acc;
  }
  return upload(c.m, fb, &op.b_grn_dev);
}

int forms_linear(PackCtx& c, PackedOp& op) {
  const ph_op_desc& d = op.d;
  const bool linear = d.kind == PH_OP_LINEAR;
  const bool no_bias = linear && d.bias == -1;  // Linear(bias=False): Swin's patch-merging reduction
  if (!c.widx_ok(d.weight) || !(c.widx_ok(d.bias) || no_bias)) return c.fail("weight index out of range");
  const int segs = linear ? 1 : 4;
  if (!linear && d.ksize != 2) return c.fail("patch conv must be 2x2 stride 2");
  if (c.weight_numel[d.weight] != (int64_t)d.cin0 * d.cout * segs || (!no_bias && c.weight_numel[d.bias] != d.cout)) return c.fail("weight size mismatch");
  if ((d.flags & PH_FLAG_RESIDUAL) && ((d.flags & PH_FLAG_SCALE_RESIDUAL) || d.src1 < 0)) return c.fail("residual epilogue needs a residual source and no layer scale");
  op.bn = gemm_choose_bn(pad16(d.cout));
  const size_t npad = n_padded(pad16(d.cout), op.bn);
  PH_TRY(c.pack([&](const auto* w, auto& out) { pack_gemm(w, d.cout, d.cin0, 0, segs, op.bn, out); }, d.weight, &op.w_dma_dev));
  PH_TRY(no_bias ? upload_zeros(c.m, npad, &op.b_dev) : c.pack(pad_vec(npad, d.cout), d.bias, &op.b_dev));
  if (linear && (d.flags & PH_FLAG_GELU) && cnblock_mlp_fits(d.cin0, pad16(d.cin0), d.cout))  // inference programs: the first Linear of a CNBlock MLP ...
    PH_TRY(c.pack([&](const auto* w, auto& out) { pack_mlp_w1(w, d.cin0, out); }, d.weight, &op.w_mlp_dev));
  else if (linear && (d.flags & PH_FLAG_SCALE_RESIDUAL) && cnblock_mlp_fits(d.cout, pad16(d.cout), d.cin0))  // ... and the second
    PH_TRY(c.pack([&](const auto* w, auto& out) { pack_mlp_w2(w, d.cout, out); }, d.weight, &op.w_mlp_dev));
  PH_TRY(forms_linear_dgrad(c, op, segs));
  // fp16 image for gemm_f16_kernel (plain fp16 precision), derived on the device
  float* image = nullptr;
  PH_TRY(derive(c.m, DERIVED_GEMM_F16_IMAGE, op.w_dma_dev, {{d.cout, d.cin0, segs, op.bn}}, &image));
  op.w_cnx_f16_dev = image;
  const ph_op_desc* g = c.i > 0 ? &c.ops[c.i - 1] : nullptr;
  if (linear && (d.flags & PH_FLAG_RESIDUAL) && !no_bias && g && g->kind == PH_OP_GRN && g->dst == d.src0 && g->cout == d.cin0 && c.widx_ok(g->bias) && c.weight_numel[g->bias] == d.cin0)
    PH_TRY(forms_grn_bias_fold(c, op, npad));
  if (d.flags & PH_FLAG_SCALE_RESIDUAL) {
    if (!c.widx_ok(d.weight2) || c.weight_numel[d.weight2] != d.cout || d.src1 < 0) return c.fail("layer-scale epilogue needs weight2 (C) and a residual source");
    PH_TRY(c.pack(pad_vec(npad, d.cout), d.weight2, &op.w2_dev));
  }
  return PH_OK;
}

// ResNet stem, Conv2d(cin0 -> cout, k7, s2, p3) with BatchNorm folded in by the host: the im2col weight image of resnet_stem_conv_kernel,
// [N block of 32][step s][lane] = W[co = 32 nb + (lane & 31)][k = s + KH (lane >> 5)] over k = (ci, ky, kx) row-major (the OIHW order itself), KH = ceil(49 cin / 2)
int forms_resnet_stem(PackCtx& c, PackedOp& op) {
  const ph_op_desc& d = op.d;
  if (!c.has_weight_and_bias(d)) return c.fail("weight index out of range");
  if (d.ksize != 7 || d.cin0 < 1 || d.cin0 > 4 || d.src0 >= 0 || d.dst2 < 0) return c.fail("resnet stem is a 7x7 stride-2 conv over the network input (1..4 channels) with a pooled slot");
  const int K = 49 * d.cin0, KH = (K + 1) / 2, coutp = pad16(d.cout), nblk = (coutp + 31) / 32;
  if (c.weight_numel[d.weight] != (int64_t)d.cout * K || c.weight_numel[d.bias] != d.cout) return c.fail("weight size mismatch");
  auto pack_img = [&](const auto* w, auto& out) {
    out.assign((size_t)resnet_stem_weight_floats(d.cin0, coutp), 0);
    for (int nb = 0; nb < nblk; ++nb)
      for (int st = 0; st < KH; ++st)
        for (int lane = 0; lane < 64; ++lane) {
          const int co = nb * 32 + (lane & 31), k = st + KH * (lane >> 5);
          if (co < d.cout && k < K) out[((size_t)nb * KH + st) * 64 + lane] = w[(size_t)co * K + k];
        }
  };
  PH_TRY(c.pack(pack_img, d.weight, &op.w_dev));
  return c.pack(pad_vec((size_t)nblk * 32, d.cout), d.bias, &op.b_dev);
}

// Conv2d(k in {1, 3}, stride 2, padding k / 2) as a row GEMM: the pack of the 3x3 stride-2 gather (mode 4, nine taps) or of the one-tap strided mode (mode 6)
int forms_conv_s2(PackCtx& c, PackedOp& op) {
  const ph_op_desc& d = op.d;
  if (!c.has_weight_and_bias(d)) return c.fail("weight index out of range");
  if ((d.ksize != 1 && d.ksize != 3) || d.src0 < 0 || d.src1 >= 0 || d.cin1 != 0) return c.fail("a stride-2 conv takes one source and kernel 1 or 3");
  const int taps = d.ksize * d.ksize, coutp = pad16(d.cout);
  if (c.weight_numel[d.weight] != (int64_t)d.cin0 * d.cout * taps || c.weight_numel[d.bias] != d.cout) return c.fail("weight size mismatch");
  op.bn = gemm_choose_bn(coutp);
  PH_TRY(c.pack([&](const auto* w, auto& out) { pack_gemm(w, d.cout, d.cin0, 0, taps, op.bn, out); }, d.weight, &op.w_dma_dev));
  return c.pack(pad_vec(n_padded(coutp, op.bn), d.cout), d.bias, &op.b_dev);
}

int forms_op(PackCtx& c, PackedOp& op) {
  switch (op.d.kind) {
    case PH_OP_POOL:
    case PH_OP_UPSAMPLE:
    case PH_OP_GELU:
    case PH_OP_ADD_RELU:
    case PH_OP_GLOBAL_MAXPOOL: return PH_OK;
    case PH_OP_RESNET_STEM: return forms_resnet_stem(c, op);
    case PH_OP_CONV_S2: return forms_conv_s2(c, op);
    case PH_OP_SCALE_ADD: return forms_scale_add(c, op);
    case PH_OP_STEM: return forms_stem(c, op);
    case PH_OP_CONV:
    case PH_OP_CONVT: return forms_conv(c, op);
    case PH_OP_INPUT_CONV:
    case PH_OP_PATCH_STEM: return forms_input_conv(c, op);
    case PH_OP_HEAD: return forms_head(c, op);
    case PH_OP_DWCONV: return forms_dwconv(c, op);
    case PH_OP_LAYERNORM:
    case PH_OP_GRN:
    case PH_OP_PATCH_MERGE: return forms_affine(c, op);
    case PH_OP_WINDOW_ATTN: return forms_window_attn(c, op);
    case PH_OP_WINDOW_ATTN_V2: return forms_window_attn_v2(c, op);
    case PH_OP_LINEAR:
    case PH_OP_PATCH_CONV: return forms_linear(c, op);
    default: return c.fail("unknown op kind");
  }
}

}  // namespace
}  // namespace ph

using namespace ph;

extern "C" ph_model* ph_model_create(const ph_op_desc* ops, int32_t n_ops, const float* const* weights, const int64_t* weight_numel, int32_t n_weights, int32_t n_slots,
                                     int32_t n_outputs) {
  if (!ops || n_ops <= 0 || n_slots <= 0) {
    set_error("ph_model_create: empty program");
    return nullptr;
  }
  if (prepare_kernels() != PH_OK || prepare_convnext_kernels() != PH_OK || prepare_f16_kernels() != PH_OK) return nullptr;
  ph_model* m = new ph_model();
  m->n_slots = n_slots;
  m->n_outputs = n_outputs;
  auto give_up = [&]() -> ph_model* {
    ph_model_destroy(m);
    return nullptr;
  };
  float* counters = nullptr;  // (uploaded as floats: all-zero bits either way; arrivals | claimed shares | departures per split-K unit)
  if (upload_zeros(m, 64, &m->zeros_dev) != PH_OK || upload_zeros(m, 3 * 4096, &counters) != PH_OK) return give_up();
  m->split_counters_dev = reinterpret_cast<unsigned*>(counters);
  // canonical parameter arena = weights[] concatenated in the given order
  m->weight_offset.resize(n_weights);
  m->weight_numel.assign(weight_numel, weight_numel + n_weights);
  for (int i = 0; i < n_weights; ++i) {
    m->weight_offset[i] = m->n_params;
    m->n_params += weight_numel[i];
  }
  if (m->n_params >= (int64_t)1 << 31) return (set_error("models with >= 2^31 parameters are not supported"), give_up());
  PackCtx c{m, ops, n_ops, weights, weight_numel, n_weights, n_outputs};
  for (c.i = 0; c.i < n_ops; ++c.i) {
    PackedOp op;
    op.d = ops[c.i];
    c.index.clear();
    if (forms_op(c, op) != PH_OK) {
      if (!c.reported) set_error("ph_model_create: op %d: %s", c.i, std::string(ph_last_error()).c_str());  // a failed allocation, copy or pack launch: name the op
      return give_up();
    }
    m->ops.push_back(op);
  }
  if (!m->derived.empty() && hipDeviceSynchronize() != hipSuccess) {  // the derived buffers were computed on the null stream
    set_error("ph_model_create: device synchronisation failed");
    return give_up();
  }
  return m;
}

extern "C" int32_t ph_gemm_case_size(void) { return (int32_t)sizeof(ph_gemm_case); }

// Test support (tests/test_gpu_row_gemm.py), not a product path: one row-GEMM launch on operands the caller owns.  The canonical weight, bias, scale and shift go
// through the product's own packers (pack_gemm, pack_convt_phase, pad_vec over n_padded), the launch through launch_gemm / launch_gemm_variant and their checks.
extern "C" int ph_debug_gemm_run(ph_gemm_case* c) {
  PH_REQUIRE(c && c->src0 && c->dst && c->weight && c->bias && c->M > 0 && c->cin0 > 0 && c->cin1 >= 0 && c->cout > 0, "ph_debug_gemm_run: bad arguments");
  PH_REQUIRE(c->mode >= 0 && c->mode <= 6 && (c->mode != 5 || ((c->ksize & 1) && c->ksize >= 1 && c->ksize <= 9)) && (c->mode != 3 || (c->cin1 == 0 && c->out_tap >= 0 && c->out_tap < 4)),
             "ph_debug_gemm_run: bad mode / kernel size / phase");
  PH_REQUIRE(c->cin1 == 0 || c->src1, "ph_debug_gemm_run: second source missing");
  if (prepare_convnext_kernels() != PH_OK) return PH_E_HIP;
  const int coutp = pad16(c->cout);
  const int bn = c->bn ? c->bn : gemm_choose_bn(coutp);
  PH_REQUIRE(bn == 128 || bn == 96 || bn == 64 || bn == 32, "ph_debug_gemm_run: unsupported N tile %d", bn);
  const size_t npad = n_padded(coutp, bn);
  struct Owned {  // what the entry allocates, freed on every way out
    std::vector<void*> p;
    ~Owned() {
      for (void* q : p) (void)hipFree(q);
    }
  } owned;
  auto up = [&](const std::vector<float>& h, const float** dev) -> int {
    void* p = nullptr;
    PH_HIP_CHECK(hipMalloc(&p, std::max<size_t>(h.size(), 4) * sizeof(float)));
    owned.p.push_back(p);
    PH_HIP_CHECK(hipMemcpy(p, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
    *dev = static_cast<const float*>(p);
    return PH_OK;
  };
  auto up_vec = [&](const float* src, const float** dev) -> int {
    std::vector<float> h;
    pad_vec(npad, c->cout)(src, h);
    return up(h, dev);
  };
  GemmArgs g{};
  std::vector<float> wp;
  if (c->mode == 3) {  // the ConvTranspose2d weight (cin, cout, 3, 3): one phase, or the four of a one-launch transposed conv
    for (int ph = 0; ph < 4; ++ph) {
      if (!c->all_phases && ph != c->out_tap) continue;
      pack_convt_phase(c->weight, c->cout, c->cin0, ph, bn, wp);
      PH_TRY(up(wp, &g.wpack_ph[ph]));
    }
    g.wpack = g.wpack_ph[c->all_phases ? 0 : c->out_tap];
    g.ntaps = (1 + (c->out_tap >> 1)) * (1 + (c->out_tap & 1));
  } else {
    const int taps = (c->mode == 0 || c->mode == 6) ? 1 : (c->mode == 1 ? 4 : (c->mode == 5 ? c->ksize * c->ksize : 9));
    pack_gemm(c->weight, c->cout, c->cin0, c->cin1, taps, bn, wp);
    PH_TRY(up(wp, &g.wpack));
  }
  PH_TRY(up_vec(c->bias, &g.bias));
  if (c->scale) PH_TRY(up_vec(c->scale, &g.scale));
  if (c->shift) PH_TRY(up_vec(c->shift, &g.shift));
  PH_TRY(up(std::vector<float>(32, 0.f), &g.zeros));  // 128 B: the least GemmArgs::zeros allows
  g.src0 = c->src0;
  g.src1 = c->src1;
  g.residual = c->residual;
  g.aux = c->aux;
  g.dst = c->dst;
  g.dst_pre = c->dst_pre;
  g.sumsq = c->sumsq;
  g.c0p = pad16(c->cin0);
  g.c1p = c->cin1 > 0 ? pad16(c->cin1) : 0;
  g.coutp = coutp;
  g.bn = bn;
  g.M = c->M;
  g.mode = c->mode;
  g.H = c->H;
  g.W = c->W;
  g.act = c->act;
  g.late_split = c->late_split;
  g.persist2 = c->persist2;
  g.all_phases = c->all_phases;
  g.ksize = c->ksize;
  g.affine_first = c->affine_first;
  g.out_patch = c->out_patch;
  g.out_tap = c->out_tap;
  g.out_H = c->out_H;
  g.out_W = c->out_W;
  g.sq_hw = c->sq_hw;
  g.sq_nseg = c->sq_nseg;
  g.tap_stride = c->tap_stride;
  const int variant = c->variant >= 0 ? c->variant : gemm_choose_variant(g);
  c->bn_used = bn;
  c->variant_used = variant;
  const int rc = c->variant >= 0 ? launch_gemm_variant(variant, g, nullptr) : launch_gemm(g, nullptr);
  PH_HIP_CHECK(hipDeviceSynchronize());
  return rc;
}

extern "C" int32_t ph_conv_run_case_size(void) { return (int32_t)sizeof(ph_conv_run_case); }

// Test support (tests/test_gpu_conv3x3.py), not a product path: one routed launch of the exact-fp32 3x3 conv on tensors the caller owns.  The canonical weight and bias go
// through pack_conv / repack_dma / pack_c16 / pad_vec over n_padded and the FORMS[] launchers with the parameters ph_model_create derives them with; the arguments are
// filled as fwd_conv3x3_f32 fills them, conv3x3_route chooses the kernel and launch_conv3x3_routed launches it.
extern "C" int ph_debug_conv3x3_run(ph_conv_run_case* c) {
  PH_REQUIRE(c && c->src0 && c->dst && c->weight && c->bias && c->B > 0 && c->H > 0 && c->W > 0 && c->cin0 > 0 && c->cin1 >= 0 && c->cout > 0, "ph_debug_conv3x3_run: bad arguments");
  const int coutp = pad16(c->cout), c0p = pad16(c->cin0), c1p = c->cin1 > 0 ? pad16(c->cin1) : 0, bn = c->bn;
  const bool n64 = bn == 64 && has_n64_form(c->cin0, c->cin1, c->cout, choose_bn(coutp));
  PH_REQUIRE(bn == choose_bn(coutp) || n64, "ph_debug_conv3x3_run: N tile %d is no packing of %d output channels", bn, coutp);
  auto on = [&](int32_t bit) { return (c->flags & bit) != 0; };
  PH_REQUIRE(on(PH_CRA_SRC1) == (c->src1 != nullptr) && on(PH_CRA_SRC1) == (c->cin1 > 0) && on(PH_CRA_POOL) == (c->dst_pool != nullptr) &&
                 on(PH_CRA_RELU_MASK) == (c->relu_mask_src != nullptr) && on(PH_CRA_HEAD) == (c->head_w != nullptr) && (!on(PH_CRA_SRC1_LOWRES) || c->src1),
             "ph_debug_conv3x3_run: flags and pointers disagree");
  PH_REQUIRE(!c->head_w || (c->head_b && c->head_dst && c->head_cout >= 1), "ph_debug_conv3x3_run: a head needs its bias, its output and a channel count");
  PH_REQUIRE((c->split_scratch_bytes > 0) == (c->split_scratch != nullptr), "ph_debug_conv3x3_run: split scratch and its size disagree");
  PH_REQUIRE(c->splitk_finish >= 0 && c->splitk_finish <= 2, "ph_debug_conv3x3_run: splitk_finish is 0, 1 or 2");
  if (prepare_kernels() != PH_OK) return PH_E_HIP;
  struct Owned {  // what the entry allocates, freed on every way out
    std::vector<void*> p;
    ~Owned() {
      for (void* q : p) (void)hipFree(q);
    }
  } owned;
  auto up = [&](const std::vector<float>& h, const float** dev) -> int {
    void* p = nullptr;
    PH_HIP_CHECK(hipMalloc(&p, std::max<size_t>(h.size(), 4) * sizeof(float)));
    owned.p.push_back(p);
    PH_HIP_CHECK(hipMemcpy(p, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
    *dev = static_cast<const float*>(p);
    return PH_OK;
  };
  auto derived = [&](DerivedKind kind, const float* src, const FormParams& fp, const float** dev) -> int {  // as derive(): FORMS[] sizes and launches it
    void* p = nullptr;
    PH_HIP_CHECK(hipMalloc(&p, (size_t)FORMS[kind].bytes(fp.p)));
    owned.p.push_back(p);
    PH_TRY(FORMS[kind].launch(src, static_cast<float*>(p), fp.p, nullptr));
    *dev = static_cast<const float*>(p);
    return PH_OK;
  };
  ConvArgs a{};
  std::vector<float> wp, tmp;
  pack_conv(c->weight, false, c->cin0, c->cin1, c->cout, bn, wp);
  PH_TRY(up(wp, &a.wpack));
  pad_vec(n_padded(coutp, bn), c->cout)(c->bias, tmp);
  PH_TRY(up(tmp, &a.bias));
  PH_TRY(up(std::vector<float>(64, 0.f), &a.zeros));
  FormParams fp;
  if (c->forms & PH_CRF_DMA) {
    PH_REQUIRE(!n64, "ph_debug_conv3x3_run: the half-empty-tile packing has no LDS-DMA form");
    repack_dma(wp, bn, tmp);
    PH_TRY(up(tmp, &a.wpack_dma));
  }
  if (c->forms & PH_CRF_WINO) {
    PH_REQUIRE(wino_form(c->cin0, c->cin1, c->cout, bn, fp), "ph_debug_conv3x3_run: no F(2,3) form for this packing");
    PH_TRY(derived(DERIVED_WINO, a.wpack, fp, &a.wpack_wino));
  }
  if (c->forms & PH_CRF_WINO2) {
    PH_REQUIRE(wino2_form(c->cin0, c->cin1, c->cout, bn, fp), "ph_debug_conv3x3_run: no F(2x2,3x3) form for this packing");
    PH_TRY(derived(DERIVED_WINO2D, a.wpack, fp, &a.wpack_wino2));
  }
  if (c->forms & PH_CRF_WINO4) {
    PH_REQUIRE(wino4_form(c->cin0, c->cin1, c->cout, bn, fp), "ph_debug_conv3x3_run: no F(4x4,3x3) form for this packing");
    PH_TRY(derived(DERIVED_WINO4, a.wpack, fp, &a.wpack_wino4));
  }
  if (c->forms & PH_CRF_W16) {
    PH_REQUIRE(w16_form(c->cin0, c->cin1, c->cout, bn, fp), "ph_debug_conv3x3_run: no wave-private form for this packing");
    PH_TRY(derived(DERIVED_W16, a.wpack, fp, &a.wpack_w16));
  }
  if (c->forms & PH_CRF_SM) PH_TRY(derived(DERIVED_SMALLMAP, a.wpack, sm_form(c->cin0, c->cin1, c->cout, bn), &a.wpack_sm));
  if (c->forms & PH_CRF_C16) {
    PH_REQUIRE(c->cin1 == 0 && c->cin0 <= 16 && c->cout <= 16, "ph_debug_conv3x3_run: conv3x3_c16's weights exist for 16 -> 16 channels from one source");
    pack_c16(c->weight, c->cout, c->cin0, tmp);
    PH_TRY(up(tmp, &a.w16));
  }
  if (c->head_w) {
    pack_head_w(c->head_w, c->head_cout, c->cout, tmp);
    PH_TRY(up(tmp, &a.head_w));
    pad_vec((size_t)c->head_cout, c->head_cout)(c->head_b, tmp);
    PH_TRY(up(tmp, &a.head_b));
    a.head_dst = c->head_dst;
    a.head_cout = c->head_cout;
    a.head_wcp = coutp;
    a.head_sigmoid = c->head_sigmoid;
  }
  const size_t n_counters = 3 * 4096;  // as ph_model_create: arrivals | claimed shares | departures of 4096 split-K units
  const float* counters = nullptr;
  PH_TRY(up(std::vector<float>(n_counters, 0.f), &counters));
  a.src0 = c->src0;
  a.src1 = c->src1;
  a.c0p = c0p, a.c1p = c1p, a.coutp = coutp;
  a.dst = c->dst;
  a.B = c->B, a.H = c->H, a.W = c->W;
  a.relu = c->relu;
  a.bn = bn;
  a.dst_pool = c->dst_pool;
  a.skip_dst = on(PH_CRA_SKIP_DST) ? 1 : 0;
  a.accumulate = on(PH_CRA_ACCUMULATE) ? 1 : 0;
  a.relu_mask_src = c->relu_mask_src;
  a.src1_lowres = on(PH_CRA_SRC1_LOWRES) ? 1 : 0;
  a.use_dma = c->use_dma, a.dma32 = c->dma32, a.use_wino = c->use_wino, a.persist = c->persist, a.use_c16 = c->use_c16, a.use_w16 = c->use_w16, a.use_wino2d = c->use_wino2d;
  a.use_wino4 = c->use_wino4, a.wino4_min_cin = c->wino4_min_cin, a.use_sm = c->use_sm, a.splitk = c->splitk;
  a.split_scratch = c->split_scratch;
  a.split_scratch_bytes = c->split_scratch_bytes;
  a.splitk_finish = c->splitk_finish;
  a.split_counters = c->splitk_finish ? reinterpret_cast<unsigned*>(const_cast<float*>(counters)) : nullptr;
  a.split_counters_n = a.split_counters ? 4096 : 0;
  int n_cu = 0;
  PH_TRY(device_cu_count(&n_cu));
  const ConvRoute r = conv3x3_route(a, n_cu);
  c->kernel = (int32_t)r.kernel;
  c->kv = r.kv;
  c->ksplit = r.ksplit;
  c->props = (r.takes_mask ? PH_CRP_MASK : 0) | (r.pools ? PH_CRP_POOLS : 0) | (r.head_w2d ? PH_CRP_HEAD_W2D : 0) | (r.head_w16 ? PH_CRP_HEAD_W16 : 0) |
             (r.folds_lowres ? PH_CRP_LOWRES : 0) | (r.head_sm ? PH_CRP_HEAD_SM : 0);
  c->n_cu = n_cu;
  c->counters_zero = 0;
  // what the forward asks the route before it hands a launch these arguments (fwd_conv3x3_f32, try_head_f32): the launcher does not check them for every kernel
  PH_REQUIRE(!(r.kernel == CONV_DMA9 && !a.wpack_dma) && !(r.kernel == CONV_C16 && !a.w16), "ph_debug_conv3x3_run: the routed kernel's weight form was not built");
  PH_REQUIRE(!a.relu_mask_src || r.takes_mask, "ph_debug_conv3x3_run: the routed kernel applies no ReLU mask");  // (the launcher checks this inside the LDS-DMA family only)
  PH_REQUIRE(!a.head_w || r.head_sm || r.head_w2d || r.head_w16, "ph_debug_conv3x3_run: the routed kernel carries no fused head");
  PH_REQUIRE(!a.src1_lowres || r.folds_lowres, "ph_debug_conv3x3_run: the routed kernel does not fold a half-resolution second source");
  PH_REQUIRE(!a.dst_pool || r.kernel != CONV_C16, "ph_debug_conv3x3_run: conv3x3_c16 has no fused pool");
  const int rc = launch_conv3x3_routed(a, r, nullptr);
  PH_HIP_CHECK(hipDeviceSynchronize());
  if (rc != PH_OK) return rc;
  std::vector<unsigned> back(n_counters);
  PH_HIP_CHECK(hipMemcpy(back.data(), counters, n_counters * sizeof(unsigned), hipMemcpyDeviceToHost));
  c->counters_zero = std::all_of(back.begin(), back.end(), [](unsigned v) { return v == 0; }) ? 1 : 0;
  return PH_OK;
}
