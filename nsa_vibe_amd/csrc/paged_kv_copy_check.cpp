// Host check of the paged copy calls' argument checks and grid sizes (paged_kv_copy.hpp): a plain host program, no HIP and no GPU, that walks
// every decline path and the sizing of accepted calls.  Built beside the library; `make paged_kv_copy_check SAN=1` builds it with
// -fsanitize=address,undefined.  Prints one line per failed expectation and exits 1, or "paged_kv_copy_check: N checks passed" and exits 0.
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "paged_kv_copy.hpp"

using namespace nsa;

static int g_checks = 0, g_failed = 0;

static void expect(bool ok, const char *what, const char *msg = "") {
    ++g_checks;
    if (!ok) {
        ++g_failed;
        printf("FAILED: %s [%s]\n", what, msg);
    }
}

struct Fixture {
    std::vector<unsigned char> mem;
    std::vector<int32_t> table, jobs;
    nsa_paged_kv_desc pkv{};
    nsa_kv_desc kv{};
    Fixture() : mem(16 * 32 + 16), table(4 * 3, -1), jobs(4 * 3, 0) {
        unsigned char *base = (unsigned char *)(((uintptr_t)mem.data() + 15) & ~(uintptr_t)15);  // never dereferenced: alignment and null only
        void **pp[8] = {&pkv.K_sel, &pkv.V_sel, &pkv.K_win, &pkv.V_win, &pkv.K_raw, &pkv.V_raw, &pkv.K_cmp, &pkv.V_cmp};
        void **kp[8] = {&kv.K_sel, &kv.V_sel, &kv.K_win, &kv.V_win, &kv.K_raw, &kv.V_raw, &kv.K_cmp, &kv.V_cmp};
        for (int i = 0; i < 8; ++i) {
            *pp[i] = base + 16 * i;
            *kp[i] = base + 16 * (8 + i);
        }
        pkv.block_table = table.data();
        pkv.table_stride = 3;
        pkv.n_pages = 7; pkv.B = 4; pkv.max_pages = 3;
        kv.B = 2; kv.S_max = 4096; kv.n_cmp_max = 255;
    }
};

struct CopyArgs {
    int b_src = 1, slot = 2, t0 = 0, t1 = 2049, G = 2, Dk = 64, Dv = 128, dtype = NSA_DT_BF16;
};

static int plan(const Fixture &f, const CopyArgs &a, PagedCopyGrid *grid, char *msg, PagedCopyParams *out = nullptr, bool null_pkv = false,
                bool null_kv = false) {
    PagedCopyParams P{};
    msg[0] = 0;
    const int rc = paged_copy_plan("paged_kv_store", null_pkv ? nullptr : &f.pkv, null_kv ? nullptr : &f.kv, a.b_src, a.slot, a.t0, a.t1, a.G, a.Dk, a.Dv,
                                   a.dtype, &P, grid, msg, 256);
    if (out) *out = P;
    return rc;
}

static void declined(const char *what, const Fixture &f, const CopyArgs &a, const char *needle, bool null_pkv = false, bool null_kv = false) {
    PagedCopyGrid g{1, 1, 1};
    char msg[256];
    const int rc = plan(f, a, &g, msg, nullptr, null_pkv, null_kv);
    expect(rc == NSA_ERR_INVALID && g.x == 0 && strstr(msg, needle) && strstr(msg, "paged_kv_store"), what, msg);
}

int main() {
    char msg[256];
    PagedCopyGrid g{};
    PagedCopyParams P{};
    {  // accepted calls and their grids
        Fixture f;
        CopyArgs a;
        expect(plan(f, a, &g, msg, &P) == NSA_OK && g.x == 9 && g.y == 16 && g.z == 1, "rows [0, 2049): nine 256-row tiles, 8 G (tensor, g) pairs", msg);
        expect(P.c0 == 0 && P.c1 == 127 && P.table_row == f.table.data() + 2 * 3, "compressed rows [0, n_cmp(2049) = 127), table row 2");
        expect(P.slab[0] == (unsigned char *)f.kv.K_sel + (int64_t)1 * 2 * 4096 * 64 * 2 && P.slab[7] == (unsigned char *)f.kv.V_cmp + (int64_t)1 * 2 * 255 * 128 * 2,
               "slab b_src: K_sel rows of Dk, V_cmp rows of Dv");
        a.t0 = 1000; a.t1 = 1040;
        expect(plan(f, a, &g, msg, &P) == NSA_OK && g.x == 2 && P.c0 == 61 && P.c1 == 64, "rows [1000, 1040): token tiles 3 and 4, compressed rows [61, 64)", msg);
        a.t0 = 1023; a.t1 = 1072;
        expect(plan(f, a, &g, msg, &P) == NSA_OK && g.x == 2 && P.c0 == 62 && P.c1 == 66, "rows [1023, 1072): compressed rows [62, 66) in two tiles", msg);
        a.t0 = 1500; a.t1 = 1500;
        expect(plan(f, a, &g, msg) == NSA_OK && g.x == 0 && g.y == 0, "t0 == t1: NSA_OK, nothing to launch", msg);
        a.t0 = 0; a.t1 = 3072;
        expect(plan(f, a, &g, msg) == NSA_OK && g.x == 12, "t1 = max_pages * 1024 is inside", msg);
        a.t1 = 1;
        expect(plan(f, a, &g, msg, &P) == NSA_OK && g.x == 1 && P.c1 == 0, "one row, no compressed row", msg);
    }
    {  // every decline path of store / load
        Fixture f;
        CopyArgs a;
        declined("null pool descriptor", f, a, "null pool descriptor", true);
        declined("null cache descriptor", f, a, "null cache descriptor", false, true);
        void **pp[8] = {&f.pkv.K_sel, &f.pkv.V_sel, &f.pkv.K_win, &f.pkv.V_win, &f.pkv.K_raw, &f.pkv.V_raw, &f.pkv.K_cmp, &f.pkv.V_cmp};
        void **kp[8] = {&f.kv.K_sel, &f.kv.V_sel, &f.kv.K_win, &f.kv.V_win, &f.kv.K_raw, &f.kv.V_raw, &f.kv.K_cmp, &f.kv.V_cmp};
        for (int i = 0; i < 8; ++i) {
            void *keep = *pp[i];
            *pp[i] = nullptr;
            declined("null pool pointer", f, a, "null pool pointer");
            *pp[i] = (unsigned char *)keep + 8;
            declined("misaligned pool", f, a, "16-byte aligned");
            *pp[i] = keep;
            keep = *kp[i];
            *kp[i] = nullptr;
            declined("null cache pointer", f, a, "null cache pointer");
            *kp[i] = (unsigned char *)keep + 2;
            declined("misaligned cache", f, a, "16-byte aligned");
            *kp[i] = keep;
        }
        f.pkv.block_table = nullptr;
        declined("null table", f, a, "null block table");
        f.pkv.block_table = (const int32_t *)((const unsigned char *)f.table.data() + 2);
        declined("misaligned table", f, a, "4-byte aligned");
        f.pkv.block_table = f.table.data();
        f.pkv.table_stride = 2;
        declined("table stride", f, a, "row stride of at least max_pages = 3");
        f.pkv.table_stride = 3;
        for (int bad : {0, -1, (1 << 20) + 1}) {
            f.pkv.max_pages = bad;
            declined("max_pages", f, a, "max_pages =");
        }
        f.pkv.max_pages = 3;
        f.pkv.n_pages = 0;
        declined("n_pages", f, a, "n_pages = 0");
        f.pkv.n_pages = 7;
        CopyArgs b = a;
        b.t0 = 5; b.t1 = 4;
        declined("t1 < t0", f, b, "0 <= t0 <= t1");
        b.t0 = -1; b.t1 = 4;
        declined("t0 < 0", f, b, "0 <= t0 <= t1");
        b = a; b.t1 = 3073;
        declined("t1 beyond the capacity", f, b, "max_pages * 1024 = 3072");
        f.kv.S_max = 2048;
        declined("t1 beyond S_max", f, a, "S_max = 2048");
        f.kv.S_max = 4096;
        f.kv.n_cmp_max = 126;
        declined("n_cmp(t1) beyond n_cmp_max", f, a, "n_cmp_max = 126");
        f.kv.n_cmp_max = 255;
        for (int dt : {NSA_DT_F32, 7, -1}) {
            b = a; b.dtype = dt;
            declined("dtype", f, b, "bf16 / f16");
        }
        for (int D : {0, 32, 96, 192, 256, -64}) {
            b = a; b.Dk = D;
            declined("Dk", f, b, "{64, 128}");
            b = a; b.Dv = D;
            declined("Dv", f, b, "{64, 128}");
        }
        for (int s : {-1, 4, 1 << 30}) {
            b = a; b.slot = s;
            declined("slot", f, b, "outside [0, B = 4)");
        }
        for (int s : {-1, 2}) {
            b = a; b.b_src = s;
            declined("b_src", f, b, "outside [0, B = 2)");
        }
        for (int G : {0, -3, 8192}) {
            b = a; b.G = G;
            declined("G", f, b, "G =");
        }
    }
    {  // copy_pages
        Fixture f;
        PagedJobsParams J{};
        expect(paged_jobs_plan("paged_kv_copy_pages", &f.pkv, f.jobs.data(), 3, 2, 64, 64, NSA_DT_F16, &J, &g, msg, 256) == NSA_OK && g.x == 3 && g.y == 16 &&
                   g.z == 4 && J.jobs == f.jobs.data() && J.n_pages == 7,
               "three jobs: grid (3, 8 G, 4)", msg);
        expect(paged_jobs_plan("paged_kv_copy_pages", &f.pkv, nullptr, 0, 2, 64, 64, NSA_DT_F16, &J, &g, msg, 256) == NSA_OK && g.x == 0, "n_jobs == 0: no launch");
        auto bad = [&](const char *what, const nsa_paged_kv_desc *pkv, const int32_t *jobs, int n, int G, int Dk, int Dv, int dt, const char *needle) {
            PagedCopyGrid gg{1, 1, 1};
            msg[0] = 0;
            const int rc = paged_jobs_plan("paged_kv_copy_pages", pkv, jobs, n, G, Dk, Dv, dt, &J, &gg, msg, 256);
            expect(rc == NSA_ERR_INVALID && gg.x == 0 && strstr(msg, needle) && strstr(msg, "paged_kv_copy_pages"), what, msg);
        };
        bad("null descriptor", nullptr, f.jobs.data(), 3, 2, 64, 64, NSA_DT_BF16, "null pool descriptor");
        bad("null jobs", &f.pkv, nullptr, 3, 2, 64, 64, NSA_DT_BF16, "null job array");
        bad("misaligned jobs", &f.pkv, (const int32_t *)((const unsigned char *)f.jobs.data() + 1), 3, 2, 64, 64, NSA_DT_BF16, "4-byte aligned");
        bad("negative n_jobs", &f.pkv, f.jobs.data(), -1, 2, 64, 64, NSA_DT_BF16, "n_jobs = -1");
        bad("dtype", &f.pkv, f.jobs.data(), 3, 2, 64, 64, NSA_DT_F32, "bf16 / f16");
        bad("Dk", &f.pkv, f.jobs.data(), 3, 2, 192, 64, NSA_DT_BF16, "{64, 128}");
        bad("Dv", &f.pkv, f.jobs.data(), 3, 2, 64, 0, NSA_DT_BF16, "{64, 128}");
        bad("G", &f.pkv, f.jobs.data(), 3, 0, 64, 64, NSA_DT_BF16, "G = 0");
        f.pkv.V_raw = nullptr;
        bad("null pool", &f.pkv, f.jobs.data(), 3, 2, 64, 64, NSA_DT_BF16, "null pool pointer");
    }
    if (g_failed) {
        printf("paged_kv_copy_check: %d of %d checks FAILED\n", g_failed, g_checks);
        return 1;
    }
    printf("paged_kv_copy_check: %d checks passed\n", g_checks);
    return 0;
}
