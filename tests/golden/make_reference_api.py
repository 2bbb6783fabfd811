#!/usr/bin/env python3
"""Writes tests/golden/reference_api.json: the facts about DRiL.jl's interface that the static checks of the Julia shim compare against (tools/check_shim.py,
tests/test_shim_static.py, tests/test_reference_golden.py), so that they run from the repository alone.  Data only:

  types            every abstract type / struct of src/ -> its declared supertype
  methods          positional argument types and `where` variables of every method of the generic functions the shim extends
  functions        the names src/ defines with `function`
  callback_locals  the keys test/test_callbacks.jl reads from the `locals` Dict at training start and at rollout start

usage: python tests/golden/make_reference_api.py <directory of a DRiL.jl checkout>     (rerun when the shim extends another generic function)"""
import json
import re
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT / "tools"))
import check_shim as cs  # noqa: E402


def main(ref: Path) -> None:
    src = cs.julia_sources(ref / "src")
    names = cs.generic_names(cs.read_shim(cs.SHIM))
    parents = {k: v for k, v in cs.type_parents(src).items() if k not in cs.BUILTIN_PARENTS}
    methods = [{"name": m["name"], "args": [t for _, t in m["args"]], "typevars": m["typevars"]} for m in cs.methods(src, names)]
    functions = sorted(set(re.findall(r"^\s*function\s+(?:\w+\.)?(\w+!?)", src, re.M)))
    t = (ref / "test" / "test_callbacks.jl").read_text()
    keys = lambda pat: sorted(set(re.findall(r":(\w+)", re.search(pat, t, re.S).group(1))))
    version = re.search(r'^version\s*=\s*"([^"]+)"', (ref / "Project.toml").read_text(), re.M).group(1)
    out = {"generator": "tests/golden/make_reference_api.py", "reference": f"DRiL.jl {version} (src/, test/test_callbacks.jl)",
           "generic_functions": sorted(names), "types": dict(sorted(parents.items())), "methods": methods, "functions": functions,
           "callback_locals": {"training_start": keys(r"OnTrainingStartCheckLocalsCallback.*?keys::Vector\{Symbol\} = \[(.*?)\]"),
                               "rollout_start": keys(r"first_keys::Vector\{Symbol\} = \[(.*?)\]")}}
    Path(__file__).with_name("reference_api.json").write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(Path(sys.argv[1]))
