// Stand-alone host check of plan_wgrad_group (csrc/gemm.hip) under AddressSanitizer + UBSan.  It includes the library's translation
// unit to reach the static planner, builds a few groups on dummy pointers and plans them at 256, 8 and 1 queues with the nine-tap
// form at its default threshold and forced.  No HIP call is made and no GPU is needed; the device code is compiled and never run.
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -fsanitize=address,undefined \
//         scripts/wgrad_plan_asan.hip -x hip masked-diffusion-model_amd/csrc/runtime.cpp -o /tmp/wgrad_plan_asan && /tmp/wgrad_plan_asan
// Exit status 0 and no sanitizer report = clean (profiles/r14_wgrad_group_plan.md).
#include "../masked-diffusion-model_amd/csrc/gemm.hip"

static mdm_gemm_desc member(int N, int H, int C0, int C1, int Cout, int stride, int ups, int k, int splitk) {
    mdm_gemm_desc d;
    memset(&d, 0, sizeof d);
    const int VH = ups ? 2 * H : H, OH = VH / stride, Cin = C0 + C1;
    void* P = reinterpret_cast<void*>(16);
    d.dtype = MDM_BF16; d.layout = 2; d.M = Cout; d.N = Cin; d.K = N * OH * OH; d.batch = 1; d.alpha = 1.0f;
    d.conv = 1; d.OH = OH; d.OW = OH; d.IH = VH; d.IW = VH; d.KH = k; d.KW = k; d.stride = stride;
    d.pad_t = k == 3 && stride == 1 ? 1 : 0; d.pad_l = d.pad_t; d.ups = ups; d.C0 = C0; d.C1 = C1; d.Ck = Cin;
    d.src0 = P; d.src1 = C1 ? P : nullptr; d.ld0 = C0; d.ld1 = C1; d.A = P; d.lda = Cout;
    d.D0 = P; d.ldd0 = Cin; d.N0 = Cin; d.out_f32 = 1; d.splitk = splitk; d.dtap = (int64_t)Cout * Cin; d.dbias = (float*)P;
    if (splitk > 1) { d.ws = P; d.ws_bytes = (int64_t)splitk * k * k * Cout * Cin * 4; }
    return d;
}

int main() {
    const int shapes[16][7] = {{8, 8, 64, 0, 64, 1, 0}, {8, 8, 64, 0, 128, 1, 0}, {4, 16, 64, 64, 64, 1, 0}, {4, 32, 128, 0, 128, 1, 0},
                               {8, 16, 64, 0, 64, 2, 0}, {4, 8, 64, 0, 64, 1, 1}, {16, 4, 256, 0, 256, 1, 0}, {4, 8, 64, 64, 128, 1, 0},
                               {4, 16, 64, 64, 128, 1, 0}, {2, 16, 128, 0, 128, 1, 1}, {4, 4, 64, 0, 128, 1, 1}, {2, 32, 64, 0, 256, 1, 0},
                               {1, 64, 64, 64, 128, 1, 0}, {2, 64, 128, 0, 128, 1, 0}, {4, 16, 8, 0, 128, 1, 0}, {4, 16, 128, 0, 8, 1, 0}};
    std::vector<mdm_gemm_desc> mixed, taps3, per_tap;
    for (int rep = 0; rep < 240; ++rep) {
        const int* s = shapes[rep % 16];
        const int nslabs = s[0] * (s[1] * (s[6] ? 2 : 1) / s[5]) * (s[1] * (s[6] ? 2 : 1) / s[5]) / 64;
        int sk = (int)(nslabs / 4.0 + 0.5); if (sk > nslabs / 8) sk = nslabs / 8; if (sk < 1) sk = 1;
        mixed.push_back(member(s[0], s[1], s[2], s[3], s[4], s[5], s[6], 3, sk));
    }
    taps3 = {member(4, 8, 64, 64, 128, 1, 0, 3, 1), member(2, 32, 64, 0, 256, 1, 0, 3, 1), member(4, 16, 8, 0, 128, 1, 0, 3, 1)};
    per_tap = {member(4, 8, 64, 0, 64, 1, 0, 3, 1), member(2, 16, 64, 0, 128, 1, 0, 1, 1), member(8, 16, 128, 0, 128, 1, 0, 3, 4)};
    int bad = 0;
    for (auto* grp : {&mixed, &taps3, &per_tap})
        for (int n_cu : {256, 8, 1})
            for (int ms : {48, 0}) {
                GroupPlan p;
                const GroupKnobs kn{n_cu, ms, 4350.0, 25000.0, true, false};
                const int rc = plan_wgrad_group(grp->data(), (int)grp->size(), kn, p);
                printf("members %zu n_cu %d min_share %d: rc %d form %d items %zu taps %zu cut %zu slots %d reduces %zu need %lld\n", grp->size(), n_cu,
                       ms, rc, (int)p.merged, p.items.size(), p.taps_table.size(), p.parts.size(), p.nslots, p.reduces.size(), (long long)p.need);
                bad += rc != 0;
            }
    GroupPlan p;       // the refusals
    mdm_gemm_desc no_ws = member(8, 16, 128, 0, 128, 1, 0, 3, 4); no_ws.ws = nullptr;
    bad += plan_wgrad_group(&no_ws, 1, GroupKnobs{256, 48, 4350.0, 25000.0, true, false}, p) == 0;
    printf("refused: %s\n", mdm_last_error());
    return bad;
}
