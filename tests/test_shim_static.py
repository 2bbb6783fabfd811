"""CPU: static checks of the Julia shim (tools/check_shim.py) — the image has no Julia, so dispatch specificity, the callback-locals keys and the
ccall surface are verified by parsing DRiLHIP.jl against the stored index of the reference's interface (tests/golden/reference_api.json) and include/*.h."""
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
TOOL = ROOT / "tools" / "check_shim.py"
SHIM = ROOT / "dril.jl_amd" / "julia" / "DRiLHIP.jl"


def _run(*args):
    return subprocess.run([sys.executable, str(TOOL), *args], capture_output=True, text=True)


def test_shim_passes_static_checks():
    r = _run()
    assert r.returncode == 0, r.stdout + r.stderr
    assert "check_shim: ok" in r.stdout


def test_checker_catches_the_round1_ambiguity(tmp_path):
    """round 1 declared `train!(agent::Agent, env::DeviceParallelEnv, ...)`: wider than the reference in argument 1, narrower in argument 2"""
    bad = tmp_path / "DRiLHIP.jl"
    import shutil
    for f in SHIM.parent.glob("DRiLHIP_*.jl"): shutil.copy(f, tmp_path / f.name)
    text = SHIM.read_text()
    assert "function train!(agent::PPOAgent, env::DeviceParallelEnv" in text
    bad.write_text(text.replace("function train!(agent::PPOAgent, env::DeviceParallelEnv", "function train!(agent::Agent, env::DeviceParallelEnv"))
    r = _run("--shim", str(bad))
    assert r.returncode == 1 and "AMBIGUOUS" in r.stdout, r.stdout


def test_checker_catches_a_missing_locals_key(tmp_path):
    import shutil
    for f in SHIM.parent.glob("DRiLHIP_*.jl"): shutil.copy(f, tmp_path / f.name)
    bad = tmp_path / "DRiLHIP.jl"
    bad.write_text(SHIM.read_text().replace(":roll_buffer, :total_fps, :callbacks, :learn_stats)", ":total_fps, :callbacks, :learn_stats)"))
    r = _run("--shim", str(bad))
    assert r.returncode == 1 and "TRAINING_START_LOCALS" in r.stdout, r.stdout


def test_checker_catches_a_wrong_ccall_width_and_arity(tmp_path):
    """a ccall whose argument is 8 bytes where the header says int32_t does not fail at run time, it corrupts: the prototype check must see it"""
    import shutil
    for f in SHIM.parent.glob("DRiLHIP_*.jl"): shutil.copy(f, tmp_path / f.name)
    text = SHIM.read_text()
    good = "ccall((:dril_env_observe, LIB[]), Int32, (Ptr{Cvoid}, Ptr{Float32}, Int32)"
    assert good in text
    for bad_sig, what in ((good.replace("Ptr{Float32}, Int32)", "Ptr{Float32}, Int64)"), "argument 3 Int64"),            # width
                          (good.replace("(Ptr{Cvoid}, Ptr{Float32}, Int32)", "(Ptr{Cvoid}, Ptr{Float32})"), "2 argument types"),   # arity
                          (good.replace("Ptr{Float32}, Int32)", "Float32, Int32)"), "argument 2 Float32"),              # pointer-ness
                          (good.replace("Ptr{Float32}, Int32)", "Ptr{Float64}, Int32)"), "argument 2 Ptr{Float64}")):  # element type
        bad = tmp_path / "DRiLHIP.jl"
        bad.write_text(text.replace(good, bad_sig))
        r = _run("--shim", str(bad))
        assert r.returncode == 1 and "ccall dril_env_observe" in r.stdout and what in r.stdout, r.stdout[-1500:]


def test_checker_catches_an_unbalanced_block(tmp_path):
    import shutil
    for f in SHIM.parent.glob("DRiLHIP_*.jl"): shutil.copy(f, tmp_path / f.name)
    extras = tmp_path / "DRiLHIP_extras.jl"
    extras.write_text(extras.read_text() + "\nfunction forgot_its_end(x)\n    x[end] + 1   # `end` inside an index is not a block end\n")
    (tmp_path / "DRiLHIP.jl").write_text(SHIM.read_text())
    r = _run("--shim", str(tmp_path / "DRiLHIP.jl"))
    assert r.returncode == 1 and "DRiLHIP_extras.jl" in r.stdout and "block openers" in r.stdout, r.stdout[-1500:]


def test_checker_catches_an_unclosed_bracket(tmp_path):
    import shutil
    for f in SHIM.parent.glob("DRiLHIP_*.jl"): shutil.copy(f, tmp_path / f.name)
    extras = tmp_path / "DRiLHIP_extras.jl"
    extras.write_text(extras.read_text() + "\nconst FORGOT = (1, 2, [3, 4)\n")
    (tmp_path / "DRiLHIP.jl").write_text(SHIM.read_text())
    r = _run("--shim", str(tmp_path / "DRiLHIP.jl"))
    assert r.returncode == 1 and "DRiLHIP_extras.jl" in r.stdout and "unexpected `)`" in r.stdout, r.stdout[-1500:]


def test_locals_lists_match_the_python_mirror(pkg):
    import re
    text = SHIM.read_text()
    keys = lambda name: tuple(re.findall(r":(\w+)", re.search(r"const " + name + r"\s*=\s*\(([^)]*)\)", text).group(1)))
    assert keys("TRAINING_START_LOCALS") == pkg.TRAINING_START_LOCALS and keys("ROLLOUT_START_LOCALS") == pkg.ROLLOUT_START_LOCALS
    sections = tuple(re.findall(r'"([^"]+)"', re.search(r"const TIMER_SECTIONS\s*=\s*\(([^)]*)\)", text).group(1)))
    assert sections == pkg.TIMER_SECTIONS
