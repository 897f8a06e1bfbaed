// Host (CPU) stage of cross-frame tracking: every pose pair score of a batch in one call.  Pure C++, no HIP.
// Replaces the Python triple loop of sleap_nn/tracking/tracker.py:513-586 (get_scores: one scoring call per (instance, candidate) pair), for the case without
// a motion model, where a candidate's feature is the past instance's own feature and a score depends on one (current, past) pair only:
//   compute_oks ................... sleap_nn/evaluation.py:644-760 as the tracker calls it: the current instance is points_gt, its bounding-box area
//                                   (compute_instance_area :625-641) the scale, np.spacing(1) added, the cocoeval normalisation
//   compute_iou ................... sleap_nn/tracking/utils.py:189-206, with its + 1s and Python's max / min (the first argument stays when a comparison is false)
//   compute_euclidean_distance .... utils.py:184-186
//   compute_cosine_sim ............ utils.py:247-252
// All arithmetic is float64 in the reference's operation order; a NaN stays NaN where NumPy gives NaN.
#include <cmath>
#include <cstdint>
#include <limits>

#include "../../include/posehip.h"

namespace ph {
void set_error(const char* fmt, ...);
}

namespace {

const double kNaN = std::numeric_limits<double>::quiet_NaN();
const double kInf = std::numeric_limits<double>::infinity();

inline double pymax(double a, double b) { return b > a ? b : a; }  // Python's max(a, b)
inline double pymin(double a, double b) { return b < a ? b : a; }

// a = the current instance (points_gt), b = the past one; n nodes of (x, y)
double oks(const double* a, const double* b, int n, double stddev) {
  // scale: prod(nanmax - nanmin) over the current instance's nodes, per axis; an axis without a number is NaN
  double lo[2] = {kNaN, kNaN}, hi[2] = {kNaN, kNaN};
  for (int i = 0; i < n; ++i)
    for (int d = 0; d < 2; ++d) {
      const double v = a[2 * i + d];
      if (std::isnan(v)) continue;
      if (std::isnan(lo[d]) || v < lo[d]) lo[d] = v;
      if (std::isnan(hi[d]) || v > hi[d]) hi[d] = v;
    }
  const double scale = (hi[0] - lo[0]) * (hi[1] - lo[1]);
  const double spread = (2 * stddev) * (2 * stddev);
  const double norm = spread * (2 * (scale + std::numeric_limits<double>::epsilon()));
  double sum = 0;
  int visible = 0;
  for (int i = 0; i < n; ++i) {
    const bool miss_gt = std::isnan(a[2 * i]) || std::isnan(a[2 * i + 1]);
    const bool miss_pr = std::isnan(b[2 * i]) || std::isnan(b[2 * i + 1]);
    if (!miss_gt) ++visible;
    double ks;
    if (miss_gt) {
      ks = 0;
    } else {
      const double dx = a[2 * i] - b[2 * i], dy = a[2 * i + 1] - b[2 * i + 1];
      const double dist = miss_pr ? kInf : dx * dx + dy * dy;
      ks = std::exp(-(dist / norm));
    }
    sum += ks;
  }
  return sum / (double)visible;  // 0 / 0 = NaN for an instance without a visible node
}

double iou(const double* a, const double* b) {
  const double ix = pymax(0, pymin(a[2], b[2]) - pymax(a[0], b[0]) + 1);
  const double iy = pymax(0, pymin(a[3], b[3]) - pymax(a[1], b[1]) + 1);
  const double inter = ix * iy;
  const double uni = (a[2] - a[0] + 1) * (a[3] - a[1] + 1) + (b[2] - b[0] + 1) * (b[3] - b[1] + 1) - inter;
  return inter / uni;
}

double neg_euclid(const double* a, const double* b, int d) {
  double s = 0;
  for (int i = 0; i < d; ++i) s += (a[i] - b[i]) * (a[i] - b[i]);
  return -std::sqrt(s);
}

double cosine(const double* a, const double* b, int d) {
  double ab = 0, aa = 0, bb = 0;
  for (int i = 0; i < d; ++i) ab += a[i] * b[i], aa += a[i] * a[i], bb += b[i] * b[i];
  return ab / (std::sqrt(aa) * std::sqrt(bb));
}

}  // namespace

extern "C" int ph_track_pose_scores(const double* cur, int32_t B, const double* hist, int32_t L, int32_t n_hist, int32_t I, int32_t N, const int32_t* counts,
                                    int32_t method, double oks_stddev, double* out) {
  if (!cur || !hist || !counts || !out) {
    ph::set_error("ph_track_pose_scores: null pointer");
    return PH_E_INVALID;
  }
  if (B < 1 || L < 1 || L > 32 || I < 1 || N < 1 || n_hist < 0 || n_hist > L) {
    ph::set_error("ph_track_pose_scores: bad shape B=%d L=%d (1..32) n_hist=%d I=%d N=%d", B, L, n_hist, I, N);
    return PH_E_INVALID;
  }
  if (method < PH_TRACK_OKS || method > PH_TRACK_COSINE || (method == PH_TRACK_IOU && N != 2)) {
    ph::set_error("ph_track_pose_scores: method %d is none of oks 0, iou 1 (N = 2: one box), euclidean_dist 2, cosine_sim 3", method);
    return PH_E_INVALID;
  }
  if ((int64_t)B * L * I * I > 0x7fffffffLL) {
    ph::set_error("ph_track_pose_scores: %lld scores per call; at most 2^31 - 1", (long long)B * L * I * I);
    return PH_E_INVALID;
  }
  for (int f = 0; f < B + L; ++f)
    if (counts[f] < 0 || counts[f] > I) {
      ph::set_error("ph_track_pose_scores: counts[%d] = %d is outside [0, %d]", f, counts[f], I);
      return PH_E_INVALID;
    }
  const size_t fs = (size_t)N * 2;  // doubles per instance
  const int D = 2 * N;
  for (int b = 0; b < B; ++b)
    for (int k = 1; k <= L; ++k) {
      double* o = out + ((size_t)b * L + (k - 1)) * I * I;
      const double* past = nullptr;
      int n_past = 0;
      if (b >= k) {
        past = cur + (size_t)(b - k) * I * fs;
        n_past = counts[b - k];
      } else if (k - b <= n_hist) {
        past = hist + (size_t)(L - (k - b)) * I * fs;
        n_past = counts[B + L - (k - b)];
      }
      const int n_cur = counts[b];
      for (int i = 0; i < I; ++i)
        for (int j = 0; j < I; ++j) {
          double v = kNaN;
          if (past && i < n_cur && j < n_past) {
            const double* a = cur + ((size_t)b * I + i) * fs;
            const double* p = past + (size_t)j * fs;
            v = method == PH_TRACK_OKS ? oks(a, p, N, oks_stddev) : method == PH_TRACK_IOU ? iou(a, p) : method == PH_TRACK_EUCLID ? neg_euclid(a, p, D) : cosine(a, p, D);
          }
          o[(size_t)i * I + j] = v;
        }
    }
  return PH_OK;
}

// The same pair functions where a candidate's feature differs per current frame (the flow-shift tracker, tracker.py:722-807: a past instance's keypoints are
// moved onto the current frame by optical flow before the feature function): hist is (B, L, I, N, 2), one candidate table per current frame.
extern "C" int ph_track_pose_scores_shifted(const double* cur, int32_t B, const double* hist, int32_t L, int32_t I, int32_t N, const int32_t* counts_cur,
                                            const int32_t* counts_hist, int32_t method, double oks_stddev, double* out) {
  if (!cur || !hist || !counts_cur || !counts_hist || !out) {
    ph::set_error("ph_track_pose_scores_shifted: null pointer");
    return PH_E_INVALID;
  }
  if (B < 1 || L < 1 || L > 32 || I < 1 || N < 1) {
    ph::set_error("ph_track_pose_scores_shifted: bad shape B=%d L=%d (1..32) I=%d N=%d", B, L, I, N);
    return PH_E_INVALID;
  }
  if (method < PH_TRACK_OKS || method > PH_TRACK_COSINE || (method == PH_TRACK_IOU && N != 2)) {
    ph::set_error("ph_track_pose_scores_shifted: method %d is none of oks 0, iou 1 (N = 2: one box), euclidean_dist 2, cosine_sim 3", method);
    return PH_E_INVALID;
  }
  if ((int64_t)B * L * I * I > 0x7fffffffLL) {
    ph::set_error("ph_track_pose_scores_shifted: %lld scores per call; at most 2^31 - 1", (long long)B * L * I * I);
    return PH_E_INVALID;
  }
  for (int f = 0; f < B; ++f)
    if (counts_cur[f] < 0 || counts_cur[f] > I) {
      ph::set_error("ph_track_pose_scores_shifted: counts_cur[%d] = %d is outside [0, %d]", f, counts_cur[f], I);
      return PH_E_INVALID;
    }
  for (int f = 0; f < B * L; ++f)
    if (counts_hist[f] < 0 || counts_hist[f] > I) {
      ph::set_error("ph_track_pose_scores_shifted: counts_hist[%d] = %d is outside [0, %d]", f, counts_hist[f], I);
      return PH_E_INVALID;
    }
  const size_t fs = (size_t)N * 2;
  const int D = 2 * N;
  for (int b = 0; b < B; ++b)
    for (int g = 0; g < L; ++g) {
      double* o = out + ((size_t)b * L + g) * I * I;
      const double* past = hist + ((size_t)b * L + g) * I * fs;
      const int n_cur = counts_cur[b], n_past = counts_hist[(size_t)b * L + g];
      for (int i = 0; i < I; ++i)
        for (int j = 0; j < I; ++j) {
          double v = kNaN;
          if (i < n_cur && j < n_past) {
            const double* a = cur + ((size_t)b * I + i) * fs;
            const double* p = past + (size_t)j * fs;
            v = method == PH_TRACK_OKS ? oks(a, p, N, oks_stddev) : method == PH_TRACK_IOU ? iou(a, p) : method == PH_TRACK_EUCLID ? neg_euclid(a, p, D) : cosine(a, p, D);
          }
          o[(size_t)i * I + j] = v;
        }
    }
  return PH_OK;
}
