// gemm_check — stand-alone driver of launch_gemm / launch_gemm_pair / launch_gemm_multi for tests/test_gemm_plan.py and tests/test_gpu_gemm.py.
// Includes the library's own dril_gemm.hip (the kernels and their selection are the product's, compiled with the product's flags), reads a case file and raw
// f32 buffer images written by tests/gemm_cases.py, runs every case TWICE and writes the whole C (and zout) buffer images of both runs back — the Python side
// knows the layouts, this side only moves bytes and launches.
//   gemm_check --plan CASEFILE            prints "<case> <target>" per case; makes no HIP call (runs on a machine without a GPU)
//   gemm_check CASEFILE DATADIR OUTDIR    one process for the whole table; every HIP status is checked, the first error ends the process (nothing is launched after it)
// Case file, whitespace separated:
//   case NAME KIND N ALLOW_SPLIT                      KIND 0 launch_gemm, 1 launch_gemm_pair (N = 2), 2 launch_gemm_multi (N = 1..4); then N lines
//   g M N K Z sAm sAk sBk sBn sCm sCn zA zB zC zBias zAux zdivB ones epi alpha zout AFILE AOFF BFILE BOFF BIASFILE AUXFILE CTOTAL COFF
// AFILE / BFILE / BIASFILE / AUXFILE name images under DATADIR ("-": none); AOFF / BOFF / COFF are element offsets of the operand inside its image; the aux image
// has C's layout (CTOTAL elements, logical start at COFF).  C and zout are CTOTAL sentinels before each run.
// build: hipcc <the library's flags> -I dril.jl_amd/csrc [-DDRIL_DEBUG_DROP_LO] -o gemm_check tests/gemm_check.hip
#include "../dril.jl_amd/csrc/dril_gemm.hip"

#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

using namespace dril;

namespace {

constexpr float kSentinel = -7777.5f;                                        // tests/gemm_cases.py SENTINEL

struct Contraction {
    GemmArgs g; int Z; int zout;
    std::string fA, fB, fBias, fAux; long long offA, offB, offC, totalC;
};
struct Case { std::string name; int kind, allow_split; std::vector<Contraction> c; };

[[noreturn]] void die(const std::string& what) { fprintf(stderr, "gemm_check: %s\n", what.c_str()); fflush(stderr); exit(1); }
#define HIP_OK(call) do { const hipError_t e_ = (call); if (e_ != hipSuccess) die(std::string(#call) + ": " + hipGetErrorString(e_)); } while (0)

std::vector<Case> read_cases(const char* path) {
    std::ifstream in(path);
    if (!in) die(std::string("cannot read ") + path);
    std::vector<Case> cases; std::string tag;
    while (in >> tag) {
        if (tag != "case") die("case file: expected `case`, got " + tag);
        Case cs; int n = 0;
        if (!(in >> cs.name >> cs.kind >> n >> cs.allow_split) || n < 1 || n > 4 || cs.kind < 0 || cs.kind > 2 || (cs.kind == 0 && n != 1) || (cs.kind == 1 && n != 2)) die("case file: bad header of " + cs.name);
        for (int i = 0; i < n; ++i) {
            Contraction c; c.g = gemm_args(); GemmArgs& g = c.g;
            if (!(in >> tag) || tag != "g") die("case file: expected `g` in " + cs.name);
            if (!(in >> g.M >> g.N >> g.K >> c.Z >> g.sAm >> g.sAk >> g.sBk >> g.sBn >> g.sCm >> g.sCn >> g.zA >> g.zB >> g.zC >> g.zBias >> g.zAux >> g.zdivB >> g.ones_n >> g.epi
                     >> g.alpha >> c.zout >> c.fA >> c.offA >> c.fB >> c.offB >> c.fBias >> c.fAux >> c.totalC >> c.offC)) die("case file: bad contraction in " + cs.name);
            g.allow_split = cs.allow_split;
            cs.c.push_back(c);
        }
        cases.push_back(cs);
    }
    return cases;
}

std::vector<float> read_image(const std::string& dir, const std::string& name) {
    std::ifstream in(dir + "/" + name, std::ios::binary | std::ios::ate);
    if (!in) die("cannot read " + dir + "/" + name);
    const std::streamsize bytes = in.tellg();
    std::vector<float> v((size_t)bytes / sizeof(float));
    in.seekg(0); in.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(v.size() * sizeof(float)));
    if (!in) die("short read of " + name);
    return v;
}
void write_image(const std::string& path, const std::vector<float>& v) {
    std::ofstream out(path, std::ios::binary);
    out.write(reinterpret_cast<const char*>(v.data()), (std::streamsize)(v.size() * sizeof(float)));
    if (!out) die("cannot write " + path);
}
float* upload(const std::string& dir, const std::string& name, std::vector<float*>& owned) {
    if (name == "-") return nullptr;
    const std::vector<float> h = read_image(dir, name);
    float* d = nullptr;
    HIP_OK(hipMalloc(&d, h.size() * sizeof(float))); owned.push_back(d);
    HIP_OK(hipMemcpy(d, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
    return d;
}

// the target(s) of a case, from the library's own selection.  Pointers matter through their 16-byte alignment only: images start 256-byte aligned like hipMalloc's
std::string plan_of(Case cs) {
    std::string out = cs.kind == 1 ? "pair:" : cs.kind == 2 ? "multi:" : "";
    for (size_t i = 0; i < cs.c.size(); ++i) {
        Contraction& c = cs.c[i];
        float* const base = reinterpret_cast<float*>((uintptr_t)1 << 20);
        c.g.A = base + c.offA; c.g.B = base + c.offB; c.g.C = base + c.offC;
        if (!gemm_prepare(c.g)) die("empty contraction in " + cs.name);
        if (i) out += "+";
        out += gemm_target_name(cs.kind == 0 ? gemm_select(c.g, c.Z) : gemm_splitk_body(c.g));
    }
    return out;
}

void run_case(const Case& cs, const std::string& data, const std::string& outdir) {
    std::vector<float*> owned; std::vector<GemmArgs> gs; std::vector<int> zs; std::vector<float*> dC, dZ;
    for (const Contraction& c : cs.c) {
        GemmArgs g = c.g;
        const float* a = upload(data, c.fA, owned); const float* b = upload(data, c.fB, owned);
        if (!a || !b) die("operand image missing in " + cs.name);
        g.A = a + c.offA; g.B = b + c.offB; g.bias = upload(data, c.fBias, owned);
        const float* aux = upload(data, c.fAux, owned); g.aux = aux ? aux + c.offC : nullptr;
        float *pc = nullptr, *pz = nullptr;
        HIP_OK(hipMalloc(&pc, (size_t)c.totalC * sizeof(float))); owned.push_back(pc);
        if (c.zout) { HIP_OK(hipMalloc(&pz, (size_t)c.totalC * sizeof(float))); owned.push_back(pz); }
        g.C = pc + c.offC; g.zout = pz ? pz + c.offC : nullptr;
        gs.push_back(g); zs.push_back(c.Z); dC.push_back(pc); dZ.push_back(pz);
    }
    for (int run = 0; run < 2; ++run) {
        for (size_t i = 0; i < cs.c.size(); ++i) {
            const std::vector<float> fill((size_t)cs.c[i].totalC, kSentinel);
            HIP_OK(hipMemcpy(dC[i], fill.data(), fill.size() * sizeof(float), hipMemcpyHostToDevice));
            if (dZ[i]) HIP_OK(hipMemcpy(dZ[i], fill.data(), fill.size() * sizeof(float), hipMemcpyHostToDevice));
        }
        if (cs.kind == 0) HIP_OK(launch_gemm(gs[0], zs[0], nullptr));
        else if (cs.kind == 1) HIP_OK(launch_gemm_pair(gs[0], zs[0], gs[1], zs[1], nullptr));
        else HIP_OK(launch_gemm_multi(gs.data(), zs.data(), (int)gs.size(), nullptr));
        HIP_OK(hipDeviceSynchronize());
        for (size_t i = 0; i < cs.c.size(); ++i) {
            std::vector<float> h((size_t)cs.c[i].totalC);
            const std::string stem = outdir + "/" + cs.name + "." + std::to_string(i);
            HIP_OK(hipMemcpy(h.data(), dC[i], h.size() * sizeof(float), hipMemcpyDeviceToHost));
            write_image(stem + ".C" + std::to_string(run) + ".bin", h);
            if (dZ[i]) {
                HIP_OK(hipMemcpy(h.data(), dZ[i], h.size() * sizeof(float), hipMemcpyDeviceToHost));
                write_image(stem + ".Z" + std::to_string(run) + ".bin", h);
            }
        }
    }
    for (float* p : owned) HIP_OK(hipFree(p));
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 3 && std::string(argv[1]) == "--plan") {
        for (const Case& cs : read_cases(argv[2])) printf("%s %s\n", cs.name.c_str(), plan_of(cs).c_str());
        return 0;
    }
    if (argc != 4) die("usage: gemm_check --plan CASEFILE | gemm_check CASEFILE DATADIR OUTDIR");
    const std::vector<Case> cases = read_cases(argv[1]);
    for (const Case& cs : cases) run_case(cs, argv[2], argv[3]);
    printf("gemm_check: %zu cases done\n", cases.size());
    return 0;
}
