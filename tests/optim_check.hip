// optim_check — stand-alone driver of the PPO optimiser tail (grad_reduce_kernel, ppo_finish_small_kernel, grad_norm_kernel, adam_kernel) for tests/test_gpu_optim.py.
// Includes the library's own dril_kernels.hip (the kernels and their four launchers are the product's, compiled with the product's flags), reads a case file and raw
// buffer images written by tests/optim_cases.py, runs every case TWICE from the same initial images and writes every buffer a kernel may write, guard zones
// included, after every step — the Python side knows the layouts and the arithmetic, this side only moves bytes and launches.
//   optim_check CASEFILE DATADIR OUTDIR    one process for the whole table; every HIP status is checked, the first error ends the process (nothing is launched after it)
// Case file, whitespace separated; F_* are f32 bit patterns in decimal (no decimal-to-binary rounding between the two sides):
//   case NAME ROUTE KIND HIDDEN PA PC L G GC NSTEPS PARAMS M V BT      ROUTE A grad_reduce -> adam | B finish_small | C grad_norm -> adam | D adam, norm_from_flat
//                                                                      KIND >= 0: the layout of that built-in env kind at [HIDDEN, HIDDEN] from the library's net_off / slab_size_*
//                                                                      (PA PC L ignored); KIND -1: the synthetic layout PA PC L, slabs rounded up to 4 floats with the 8 statistics last
//                                                                      PARAMS M V BT: initial images under DATADIR (P, P, P, 4 floats)
//   step PARITY CLEAR USE_STATS HAS_KL HAS_MAX NSAMPLES F_TARGET_KL F_MAX_NORM F_LR F_BETA1 F_BETA2 F_EPS F_ENT F_VF IN0 IN1      NSTEPS of them
//                                                                      CLEAR: zero stop_flag and nan_flag first (dril_ppo_update at the start of an update)
//                                                                      routes A, B: IN0 / IN1 = actor / critic slab images (G slab_a, GC slab_c floats); C, D: IN0 = flat (P + 8), IN1 = "-"
// OUTDIR/layouts.txt: "NAME P PA PC SLAB_A SLAB_C" per case, the numbers the driver used.
// OUTDIR/NAME.run{0,1}.bin, per step: norm_partials (f64), flat, params, m, v, bt, norm_out, step_stats (f32) — each as [kGuard | logical | kGuard] —, then nan_flag, stop_flag (i32).
// Before every step flat (routes A, B), norm_partials, norm_out and step_stats are sentinels throughout: what a kernel had to write and did not stays visible.
// build: hipcc <the library's flags> <KERNELS_EXTRA> -I dril.jl_amd/csrc -o optim_check tests/optim_check.hip
#include "../dril.jl_amd/csrc/dril_kernels.hip"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

namespace dril {   // launch_ppo_grad (dril_kernels.hip) refers to the gradient kernels' translation units, which this driver neither links nor runs
hipError_t launch_ppo_grad_f32(int, int, const GradArgs&, hipStream_t) { return hipErrorNotSupported; }
hipError_t launch_ppo_grad_pair(int, const GradArgs&, hipStream_t) { return hipErrorNotSupported; }
hipError_t launch_ppo_grad_wide(int, int, const GradArgs&, hipStream_t) { return hipErrorNotSupported; }
}  // namespace dril

using namespace dril;

namespace {

constexpr float kSentinel = -7777.5f;                                        // tests/optim_cases.py SENTINEL (f32 and f64 buffers alike)
constexpr size_t kGuard = 64;                                                // sentinel elements before and after every buffer a kernel writes
constexpr size_t kSlack = 1024;                                              // NaN floats around every read-only input image

struct Step {
    int parity, clear, use_stats, has_kl, has_max; double n_samples;
    float target_kl, max_norm, lr, beta1, beta2, eps, ent, vf; std::string in0, in1;
};
struct Case { std::string name, params, m, v, bt; char route; int kind, hidden, Pa, Pc, L, G, Gc; std::vector<Step> steps; };

[[noreturn]] void die(const std::string& what) { fprintf(stderr, "optim_check: %s\n", what.c_str()); fflush(stderr); exit(1); }
#define HIP_OK(call) do { const hipError_t e_ = (call); if (e_ != hipSuccess) die(std::string(#call) + ": " + hipGetErrorString(e_)); } while (0)

bool read_f32_bits(std::istream& in, float& f) { uint32_t u; if (!(in >> u)) return false; std::memcpy(&f, &u, 4); return true; }

std::vector<Case> read_cases(const char* path) {
    std::ifstream in(path);
    if (!in) die(std::string("cannot read ") + path);
    std::vector<Case> cases; std::string tag;
    while (in >> tag) {
        if (tag != "case") die("case file: expected `case`, got " + tag);
        Case c; int n = 0;
        if (!(in >> c.name >> c.route >> c.kind >> c.hidden >> c.Pa >> c.Pc >> c.L >> c.G >> c.Gc >> n >> c.params >> c.m >> c.v >> c.bt) || n < 1 || n > 64 ||
            c.route < 'A' || c.route > 'D' || c.G < 1 || c.Gc < 1) die("case file: bad header of " + c.name);
        for (int i = 0; i < n; ++i) {
            Step s;
            if (!(in >> tag) || tag != "step") die("case file: expected `step` in " + c.name);
            if (!(in >> s.parity >> s.clear >> s.use_stats >> s.has_kl >> s.has_max >> s.n_samples) || !read_f32_bits(in, s.target_kl) || !read_f32_bits(in, s.max_norm) ||
                !read_f32_bits(in, s.lr) || !read_f32_bits(in, s.beta1) || !read_f32_bits(in, s.beta2) || !read_f32_bits(in, s.eps) || !read_f32_bits(in, s.ent) ||
                !read_f32_bits(in, s.vf) || !(in >> s.in0 >> s.in1)) die("case file: bad step in " + c.name);
            c.steps.push_back(s);
        }
        cases.push_back(c);
    }
    return cases;
}

std::vector<float> read_image(const std::string& dir, const std::string& name, size_t want) {
    std::ifstream in(dir + "/" + name, std::ios::binary | std::ios::ate);
    if (!in) die("cannot read " + dir + "/" + name);
    const std::streamsize bytes = in.tellg();
    if ((size_t)bytes != want * sizeof(float)) die(name + ": " + std::to_string((long long)bytes) + " bytes, the layout needs " + std::to_string(want * sizeof(float)));
    std::vector<float> v(want);
    in.seekg(0); in.read(reinterpret_cast<char*>(v.data()), bytes);
    if (!in) die("short read of " + name);
    return v;
}

// a device buffer of n logical elements between two guard zones
template <class T> struct Guarded {
    T* base = nullptr; size_t n = 0;
    void alloc(size_t n_) { n = n_; HIP_OK(hipMalloc(&base, total() * sizeof(T))); }
    size_t total() const { return n + 2 * kGuard; }
    T* p() const { return base + kGuard; }
    void fill(const T* logical) const {                                       // logical == nullptr: sentinels throughout
        std::vector<T> h(total(), (T)kSentinel);
        if (logical) std::memcpy(h.data() + kGuard, logical, n * sizeof(T));
        HIP_OK(hipMemcpy(base, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    }
    void dump(std::ofstream& out) const {
        std::vector<T> h(total());
        HIP_OK(hipMemcpy(h.data(), base, h.size() * sizeof(T), hipMemcpyDeviceToHost));
        out.write(reinterpret_cast<const char*>(h.data()), (std::streamsize)(h.size() * sizeof(T)));
    }
    void release() { if (base) HIP_OK(hipFree(base)); base = nullptr; }
};

// a read-only input: the image between two runs of NaN (a kernel that reads outside the image turns its result NaN)
struct Input {
    float* base = nullptr;
    const float* p() const { return base + kSlack; }
    void upload(const std::vector<float>& img) {
        std::vector<float> h(img.size() + 2 * kSlack, NAN);
        std::memcpy(h.data() + kSlack, img.data(), img.size() * sizeof(float));
        HIP_OK(hipMalloc(&base, h.size() * sizeof(float)));
        HIP_OK(hipMemcpy(base, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    void release() { if (base) HIP_OK(hipFree(base)); base = nullptr; }
};

struct Layout { int P, Pa, Pc, slab_a, slab_c; };
Layout layout_of(const Case& c) {
    Layout l;
    if (c.kind >= 0) {
        const EnvKindInfo* k = env_kind_info(c.kind);
        if (!k) die("no built-in env kind " + std::to_string(c.kind));
        const NetOff actor = net_off(0, k->D, c.hidden, c.hidden, k->A), critic = net_off(actor.end, k->D, c.hidden, c.hidden, 1);   // dril_create
        l.Pa = actor.end; l.Pc = critic.end - actor.end; l.P = critic.end + (k->discrete ? 0 : k->A);
        l.slab_a = slab_size_actor(*k, c.hidden); l.slab_c = slab_size_critic(*k, c.hidden);
    } else {
        if (c.Pa < 1 || c.Pc < 1 || c.L < 0) die("bad synthetic layout in " + c.name);
        l.Pa = c.Pa; l.Pc = c.Pc; l.P = c.Pa + c.Pc + c.L;
        l.slab_a = (c.Pa + c.L + 8 + 3) / 4 * 4; l.slab_c = (c.Pc + 8 + 3) / 4 * 4;
    }
    return l;
}

void run_case(const Case& c, const std::string& data, const std::string& outdir, std::ofstream& layouts, hipStream_t stream) {
    const Layout l = layout_of(c);
    const size_t P = (size_t)l.P;
    const bool slabs = c.route == 'A' || c.route == 'B';
    if (c.route == 'B' && l.P > 16384) die(c.name + ": ppo_finish_small_kernel holds at most 16384 parameters");
    if (l.slab_a < l.Pa + (l.P - l.Pa - l.Pc) + 8 || l.slab_c < l.Pc + 8) die(c.name + ": a slab smaller than its contents");
    layouts << c.name << " " << l.P << " " << l.Pa << " " << l.Pc << " " << l.slab_a << " " << l.slab_c << "\n";
    layouts.flush();

    const int n_partials = (int)((P + 31) / 32);                               // dril_create
    Guarded<float> flat, params, m, v, bt, norm_out, step_stats; Guarded<double> norm_partials;
    flat.alloc(P + 8); params.alloc(P); m.alloc(P); v.alloc(P); bt.alloc(4); norm_out.alloc(1); step_stats.alloc(12); norm_partials.alloc((size_t)n_partials);
    int* flags = nullptr;                                                      // {nan_flag, stop_flag}
    HIP_OK(hipMalloc(&flags, 2 * sizeof(int)));
    const std::vector<float> p0 = read_image(data, c.params, P), m0 = read_image(data, c.m, P), v0 = read_image(data, c.v, P), bt0 = read_image(data, c.bt, 4);
    std::vector<Input> in0(c.steps.size()), in1(c.steps.size());
    for (size_t i = 0; i < c.steps.size(); ++i) {
        if (slabs) {
            in0[i].upload(read_image(data, c.steps[i].in0, (size_t)c.G * l.slab_a));
            in1[i].upload(read_image(data, c.steps[i].in1, (size_t)c.Gc * l.slab_c));
        } else in0[i].upload(read_image(data, c.steps[i].in0, P + 8));
    }

    for (int run = 0; run < 2; ++run) {
        std::ofstream out(outdir + "/" + c.name + ".run" + std::to_string(run) + ".bin", std::ios::binary);
        if (!out) die("cannot write the outputs of " + c.name);
        params.fill(p0.data()); m.fill(m0.data()); v.fill(v0.data()); bt.fill(bt0.data());
        const int zero[2] = {0, 0};                                            // (blocking copies: complete before the next launch on `stream`)
        HIP_OK(hipMemcpy(flags, zero, sizeof(zero), hipMemcpyHostToDevice));
        for (size_t i = 0; i < c.steps.size(); ++i) {
            const Step& s = c.steps[i];
            if (s.clear) HIP_OK(hipMemcpy(flags, zero, sizeof(zero), hipMemcpyHostToDevice));
            if (slabs) flat.fill(nullptr);
            else { std::vector<float> f(P + 8); HIP_OK(hipMemcpy(f.data(), in0[i].p(), f.size() * sizeof(float), hipMemcpyDeviceToHost)); flat.fill(f.data()); }
            norm_partials.fill(nullptr); norm_out.fill(nullptr); step_stats.fill(nullptr);

            ReduceArgs r{};
            r.slabs_actor = in0[i].p(); r.slabs_critic = slabs ? in1[i].p() : nullptr; r.slab_a = l.slab_a; r.slab_c = l.slab_c; r.G = c.G; r.Gc = c.Gc;
            r.P = l.P; r.Pa = l.Pa; r.Pc = l.Pc; r.flat = flat.p(); r.norm_partials = norm_partials.p(); r.n_samples_local = s.n_samples; r.stop_flag = flags + 1;
            AdamArgs ad{};
            ad.params = params.p(); ad.m = m.p(); ad.v = v.p(); ad.flat = flat.p(); ad.P = l.P; ad.norm_partials = norm_partials.p(); ad.n_partials = n_partials;
            ad.norm_from_flat = c.route == 'D' ? 1 : 0; ad.bt = bt.p(); ad.step_parity = s.parity;
            ad.beta1 = s.beta1; ad.beta2 = s.beta2; ad.eps = s.eps; ad.lr = s.lr; ad.max_grad_norm = s.max_norm; ad.target_kl = s.target_kl; ad.ent_coef = s.ent; ad.vf_coef = s.vf;
            ad.has_max_grad_norm = s.has_max; ad.has_target_kl = s.has_kl; ad.use_stats = s.use_stats;
            ad.step_stats = step_stats.p(); ad.norm_out = norm_out.p(); ad.nan_flag = flags; ad.stop_flag = flags + 1; ad.stop_flag_w = flags + 1;

            if (c.route == 'A') { HIP_OK(launch_grad_reduce(r, stream)); HIP_OK(launch_adam(ad, stream)); }
            else if (c.route == 'B') HIP_OK(launch_finish_small(r, ad, stream));
            else if (c.route == 'C') { HIP_OK(launch_grad_norm(flat.p(), l.P, norm_partials.p(), flags + 1, stream)); HIP_OK(launch_adam(ad, stream)); }
            else HIP_OK(launch_adam(ad, stream));
            HIP_OK(hipStreamSynchronize(stream));

            norm_partials.dump(out); flat.dump(out); params.dump(out); m.dump(out); v.dump(out); bt.dump(out); norm_out.dump(out); step_stats.dump(out);
            int hf[2];
            HIP_OK(hipMemcpy(hf, flags, sizeof(hf), hipMemcpyDeviceToHost));
            out.write(reinterpret_cast<const char*>(hf), sizeof(hf));
            if (!out) die("cannot write the outputs of " + c.name);
        }
    }
    for (Input& x : in0) x.release();
    for (Input& x : in1) x.release();
    flat.release(); params.release(); m.release(); v.release(); bt.release(); norm_out.release(); step_stats.release(); norm_partials.release();
    HIP_OK(hipFree(flags));
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 4) die("usage: optim_check CASEFILE DATADIR OUTDIR");
    const std::vector<Case> cases = read_cases(argv[1]);
    std::ofstream layouts(std::string(argv[3]) + "/layouts.txt");
    if (!layouts) die("cannot write layouts.txt");
    hipStream_t stream;
    HIP_OK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    for (const Case& c : cases) run_case(c, argv[2], argv[3], layouts, stream);
    HIP_OK(hipStreamDestroy(stream));
    printf("optim_check: %zu cases done\n", cases.size());
    return 0;
}
