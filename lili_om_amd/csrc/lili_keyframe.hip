// Keyframe hand-over: what LidarOdometry::run does once it has a pose (L/src/LidarOdometry.cpp:565-586, 624-650, 675-680; the same text in R/).
//   lili_kf_rule_*            the keyframe decision                  (host, no context)
//   lili_pose_relative        computeRelative, L:444-480            (host, no context)
//   k_keyframe_undistort      undistortion(cloud, trans, quat), L:178-199, for the keyframe's three clouds in ONE launch: a streaming kernel, one point per lane,
//                             12-48 bytes in and 16 out, f64 arithmetic; the slerp's acos and sin once per workgroup (as k_livox_prep), no other LDS
//   lili_keyframe_undistort   the kernel on a caller's clouds;  lili_frontend_keyframe: on the last extraction's own device lists (publishCloudLast, L:624-650)
#include "lili_ctx.h"
#include "lili_device_cloud.h"
#include "lili_device_math.h"

namespace lili {

// One cloud of the launch, column by column: x y z at `xyz`, the time channel and the published 4th float wherever their columns lie (aux == nullptr: 0), `first` = its
// position in the concatenation (seg_of), move = 0: the rows are only converted.
struct KfSeg { const unsigned char* xyz; const unsigned char* time; const unsigned char* aux; float4* out; long long first; int xyz_stride, time_stride, aux_stride, move; };
struct KfArgs { KfSeg seg[3]; double t[3]; double q[4]; long long total; int general; };

// (int) of a float as the reference's x86 build converts it: NaN and every value outside int give INT_MIN (cvttss2si)
__device__ __forceinline__ int x86_float_to_int(float f) { return (f >= -2147483648.f && f < 2147483648.f) ? (int)f : (-2147483647 - 1); }

__global__ __launch_bounds__(256) void k_keyframe_undistort(const KfArgs A) {
    __shared__ SlerpConst slerp_s;
    const dq q{A.q[0], A.q[1], A.q[2], A.q[3]};
    if (A.general) {      // (uniform over the launch)
        if (threadIdx.x == 0) slerp_s = qslerp_prepare(q);
        __syncthreads();
    }
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= A.total) return;
    const int s = seg_of(A.seg, 3, i);
    const KfSeg S = A.seg[s];
    const size_t r = (size_t)(i - S.first);
    const float* p = reinterpret_cast<const float*>(S.xyz + r * (size_t)S.xyz_stride);
    const float x = p[0], y = p[1], z = p[2];
    const float aux = S.aux ? *reinterpret_cast<const float*>(S.aux + r * (size_t)S.aux_stride) : 0.f;
    float ox = x, oy = y, oz = z;
    if (S.move) {
        const float I = *reinterpret_cast<const float*>(S.time + r * (size_t)S.time_stride);
        const int line = x86_float_to_int(I);                                   // L:181
        const double dt_i = (double)(I - (float)line);                          // L:182: a float subtraction, widened
        double ratio = dt_i / 0.1;                                              // L:183
        if (ratio > 1) ratio = 1;                                               // L:185-186 (no lower bound; NaN passes)
        if (!A.general) {
            // quat = (1, 0, 0, 0): the slerp's linear branch gives a zero vector part, q_si * p is p itself for finite p — and NaN in all three for any other p
            // (Eigen's u.cross(v) multiplies every component of v by zero) or a ratio that is not finite (NaN, or -inf: the slerp's weights are then inf and -inf)
            if (isfinite(x) && isfinite(y) && isfinite(z) && isfinite(ratio)) {
                ox = (float)((double)x + ratio * A.t[0]); oy = (float)((double)y + ratio * A.t[1]); oz = (float)((double)z + ratio * A.t[2]);      // L:191-197
            } else ox = oy = oz = __builtin_nanf("");
        } else {
            const dq qs = qslerp_identity(ratio, q, slerp_s);                   // L:188-189
            const d3 v = qrot(qs, d3{(double)x, (double)y, (double)z}) + ratio * d3{A.t[0], A.t[1], A.t[2]};
            ox = (float)v.x; oy = (float)v.y; oz = (float)v.z;
        }
    }
    S.out[r] = make_float4(ox, oy, oz, aux);
}

}  // namespace lili

namespace lili_detail {
struct KeyframeBuffers : ExtState {
    DevBuf stage[3];      // pageable host clouds of lili_keyframe_undistort, as they are
    DevBuf out[3];        // lili_frontend_keyframe: edge, surf, full
    int n[3] = {0, 0, 0};
    bool have = false;
};
}  // namespace lili_detail
static lili_detail::KeyframeBuffers* kf_of(lili_ctx* ctx) { return ext_of<lili_detail::KeyframeBuffers>(ctx, lili_ctx::kExtKeyframe); }

// the launch: segments with n > 0 only count; nothing enqueued for an empty concatenation
static int kf_launch(lili_ctx* ctx, const lili_kf_source src[3], float4* const out[3], const double t_rel[3], const double q_rel[4], bool deskew) {
    KfArgs A{};
    long long total = 0;
    for (int k = 0; k < 3; k++) {
        KfSeg& S = A.seg[k];
        S.xyz = src[k].xyz; S.time = src[k].time; S.aux = src[k].aux; S.out = out[k]; S.first = total;
        S.xyz_stride = src[k].xyz_stride; S.time_stride = src[k].time_stride; S.aux_stride = src[k].aux_stride; S.move = deskew ? 1 : 0;
        total += src[k].n;
    }
    if (total == 0) return LILI_OK;
    A.total = total;
    for (int c = 0; c < 3; c++) A.t[c] = t_rel ? t_rel[c] : 0.0;
    A.q[0] = 1.0;
    A.general = 0;
    if (q_rel && !(q_rel[0] == 1.0 && q_rel[1] == 0.0 && q_rel[2] == 0.0 && q_rel[3] == 0.0)) { for (int c = 0; c < 4; c++) A.q[c] = q_rel[c]; A.general = 1; }
    hipLaunchKernelGGL(k_keyframe_undistort, dim3(nblocks(total, 256)), dim3(256), 0, ctx->stream, A);
    HIPCHK(hipGetLastError());
    return LILI_OK;
}

extern "C" {

void lili_kf_rule_reset(lili_kf_rule_state* st) {
    if (!st) return;
    std::memset(st, 0, sizeof(*st));
    st->q_last[0] = 1.0;      // quat_last_kF = Identity, trans_last_kf = Zero (L:74-75)
    st->kf = 1;               // bool kf = true (L:71)
}

int lili_kf_rule_step(lili_kf_rule_state* st, const double t[3], const double q[4], int matched) {
    if (!st) return LILI_E_ARG;
    if (st->n_frames == 0) {      // !system_initialized: savePoses + checkInitialization (L:662-666)
        st->n_frames = 1;
        return LILI_KF_FIRST;
    }
    if (!t || !q) return LILI_E_ARG;
    if (matched) {                // updateTransformationWithCeres did not return early (L:485-488)
        const double dx = t[0] - st->t_last[0], dy = t[1] - st->t_last[1], dz = t[2] - st->t_last[2];
        const double dis = std::sqrt(dx * dx + dy * dy + dz * dz);                                      // L:573
        const double* l = st->q_last;
        const double n2 = l[1] * l[1] + l[2] * l[2] + l[3] * l[3] + l[0] * l[0];                        // squaredNorm over coeffs() x, y, z, w
        double iw = 0, ix = 0, iy = 0, iz = 0;
        if (n2 > 0) { iw = l[0] / n2; ix = -l[1] / n2; iy = -l[2] / n2; iz = -l[3] / n2; }
        const double w = iw * q[0] - ix * q[1] - iy * q[2] - iz * q[3];                                 // (quat_last_kF.inverse() * quatCur).w()
        const double ang = 2 * std::acos(w);                                                            // L:574 (NaN for |w| > 1: compares false)
        const uint64_t n = (uint64_t)st->n_frames, since = n - (uint64_t)st->kf_num;                    // size_t arithmetic, as the node's
        if ((((dis > 0.2 || ang > 0.1) && (since > 1)) || (since > 2)) || n <= 1) {                     // L:575
            st->kf = 1;
            for (int c = 0; c < 3; c++) st->t_last[c] = t[c];
            for (int c = 0; c < 4; c++) st->q_last[c] = q[c];
        } else st->kf = 0;
    }
    st->n_frames += 1;                             // savePoses (L:673)
    if (st->kf) st->kf_num = st->n_frames;          // L:675-676
    return st->kf ? LILI_KF_YES : LILI_KF_NO;
}

int lili_pose_relative(const double t_prev[3], const double q_prev[4], const double t_cur[3], const double q_cur[4], double t_rel[3], double q_rel[4]) {
    if (!t_prev || !q_prev || !t_cur || !q_cur || !t_rel || !q_rel) return LILI_E_ARG;
    const double n2 = q_prev[1] * q_prev[1] + q_prev[2] * q_prev[2] + q_prev[3] * q_prev[3] + q_prev[0] * q_prev[0];
    double aw = 0, ax = 0, ay = 0, az = 0;                                                              // quaternion1.inverse()
    if (n2 > 0) { aw = q_prev[0] / n2; ax = -q_prev[1] / n2; ay = -q_prev[2] / n2; az = -q_prev[3] / n2; }
    const double bw = q_cur[0], bx = q_cur[1], by = q_cur[2], bz = q_cur[3];
    const double rw = aw * bw - ax * bx - ay * by - az * bz, rx = aw * bx + ax * bw + ay * bz - az * by;      // L:470
    const double ry = aw * by + ay * bw + az * bx - ax * bz, rz = aw * bz + az * bw + ax * by - ay * bx;
    const double vx = t_cur[0] - t_prev[0], vy = t_cur[1] - t_prev[1], vz = t_cur[2] - t_prev[2];            // L:471: v + w * (2 u x v) + u x (2 u x v)
    double cx = ay * vz - az * vy, cy = az * vx - ax * vz, cz = ax * vy - ay * vx;
    cx = cx + cx; cy = cy + cy; cz = cz + cz;
    const double ex = ay * cz - az * cy, ey = az * cx - ax * cz, ez = ax * cy - ay * cx;
    q_rel[0] = rw; q_rel[1] = rx; q_rel[2] = ry; q_rel[3] = rz;
    t_rel[0] = (vx + cx * aw) + ex; t_rel[1] = (vy + cy * aw) + ey; t_rel[2] = (vz + cz * aw) + ez;
    return LILI_OK;
}

int lili_keyframe_undistort(lili_ctx* ctx, const lili_cloud* const clouds[3], const int time_offset[3], const double t_rel[3], const double q_rel[4],
                            lili_feature_out out[3]) {
    if (!ctx) return LILI_E_ARG;
    ARGCHK(clouds && time_offset && t_rel && out, "keyframe_undistort: null argument");
    ARGCHK(finite_n(t_rel, 3) && (!q_rel || finite_n(q_rel, 4)), "keyframe_undistort: non-finite relative pose");
    // every check before anything is enqueued
    for (int k = 0; k < 3; k++) {
        const lili_cloud* c = clouds[k];
        if (!c || c->n == 0) continue;
        TRY(lili_cloud_check(ctx, *c, "keyframe_undistort"));
        ARGCHK(c->aux_offset < 0 || c->aux_offset % 4 == 0, "keyframe_undistort: aux_offset outside the point or no multiple of 4");
        ARGCHK(time_offset[k] >= 0 && time_offset[k] % 4 == 0 && (size_t)time_offset[k] + 4 <= c->stride, "keyframe_undistort: time_offset outside the point or no multiple of 4");
        ARGCHK((reinterpret_cast<uintptr_t>(c->data) & 3) == 0, "keyframe_undistort: cloud not 4-byte aligned");
        ARGCHK(out[k].data && out[k].mem == LILI_MEM_DEVICE && out[k].stride == 16 && out[k].capacity >= c->n, "keyframe_undistort: out must be a device buffer of 16-byte rows with room for the cloud");
        ARGCHK((reinterpret_cast<uintptr_t>(out[k].data) & 15) == 0, "keyframe_undistort: out not 16-byte aligned");
    }
    HIPCHK(hipSetDevice(ctx->device));
    auto* K = kf_of(ctx);
    lili_kf_source src[3];
    float4* dst[3] = {nullptr, nullptr, nullptr};
    for (int k = 0; k < 3; k++) {
        const lili_cloud* c = clouds[k];
        out[k].count = 0;
        if (!c || c->n == 0) continue;
        const unsigned char* base = nullptr;
        TRY(lili_cloud_sources(ctx, K->stage[k], c, 1, kReadPinnedInPlace, &base));
        src[k].xyz = base; src[k].time = base + time_offset[k]; src[k].aux = c->aux_offset >= 0 ? base + c->aux_offset : nullptr;
        src[k].xyz_stride = src[k].time_stride = src[k].aux_stride = (int)c->stride; src[k].n = (int)c->n;
        dst[k] = static_cast<float4*>(out[k].data);
        out[k].count = c->n;
    }
    return kf_launch(ctx, src, dst, t_rel, q_rel, true);
}

int lili_frontend_keyframe(lili_ctx* ctx, int flavour, const double t_rel[3], const double q_rel[4], int deskew, lili_cloud* edge, lili_cloud* surf, lili_cloud* full) {
    if (!ctx) return LILI_E_ARG;
    ARGCHK(flavour == LILI_VARIANT_LIVOX || flavour == LILI_VARIANT_ROT, "frontend_keyframe: flavour must be LILI_VARIANT_LIVOX or LILI_VARIANT_ROT");
    ARGCHK(!deskew || (t_rel && finite_n(t_rel, 3) && (!q_rel || finite_n(q_rel, 4))), "frontend_keyframe: deskew needs a finite relative pose");
    lili_kf_source src[3];
    TRY(flavour == LILI_VARIANT_LIVOX ? lili_extract_livox_kf_sources(ctx, src) : lili_extract_rot_kf_sources(ctx, src));
    HIPCHK(hipSetDevice(ctx->device));
    auto* K = kf_of(ctx);
    K->have = false;
    float4* dst[3];
    for (int k = 0; k < 3; k++) {
        HIPCHK(K->out[k].ensure((size_t)std::max(src[k].n, 1) * sizeof(float4)));
        dst[k] = K->out[k].as<float4>();
        K->n[k] = src[k].n;
    }
    TRY(kf_launch(ctx, src, dst, t_rel, q_rel, deskew != 0));
    K->have = true;
    lili_cloud* views[3] = {edge, surf, full};
    for (int k = 0; k < 3; k++) if (views[k]) *views[k] = lili_cloud{K->out[k].p, (size_t)K->n[k], 16, 12, LILI_MEM_DEVICE};
    return LILI_OK;
}

int lili_frontend_keyframe_get(lili_ctx* ctx, int kind, lili_feature_out* out) {
    if (!ctx) return LILI_E_ARG;
    ARGCHK(kind >= 0 && kind < 3 && out, "frontend_keyframe_get: kind is 0 (edge), 1 (surf) or 2 (full)");
    auto* K = kf_of(ctx);
    if (!K->have) return ctx->fail(LILI_E_STATE, "frontend_keyframe_get: run lili_frontend_keyframe first");
    ARGCHK(out->mem == LILI_MEM_HOST || out->mem == LILI_MEM_DEVICE, "frontend_keyframe_get: bad mem");
    out->count = (size_t)K->n[kind];
    const size_t rows = std::min(out->count, out->capacity);
    if (rows == 0) return LILI_OK;
    ARGCHK(out->data && out->stride >= 16, "frontend_keyframe_get: out needs data and a stride of at least 16");
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipMemcpy2DAsync(out->data, out->stride, K->out[kind].p, 16, 16, rows, out->mem == LILI_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return LILI_OK;
}

}  // extern "C"
