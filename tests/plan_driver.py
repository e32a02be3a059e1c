"""pfnl_amd/csrc/launch_plan.h as a host program (no GPU): one line "ncu T B H W Hfull nl_fits key=value ..." in, the pfnl_plan text of
that device, shape and option setting out, followed by " | " and the plan's fields the text does not carry.  The keys and values are
pfnl_set_option's (the header's own table).  Used by tests/test_plan_host.py and by the GPU test that ties the library to the header."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

DRIVER = r"""
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include "launch_plan.h"

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        pfnl::Options opt;
        pfnl::PlanFacts facts;
        int B, H, W, Hfull, nl_fits;
        if (!(in >> facts.ncu >> facts.num_frames >> B >> H >> W >> Hfull >> nl_fits)) return 2;
        std::string kv;
        while (in >> kv) {
            const size_t eq = kv.find('=');
            const pfnl::OptionSpec* o = eq == std::string::npos ? nullptr : pfnl::find_option(kv.substr(0, eq));
            if (!o || !o->set_named(opt, kv.substr(eq + 1))) return 3;
        }
        const pfnl::TrunkPlan pl = pfnl::trunk_plan(opt, facts, B, H, W, Hfull, nl_fits != 0);
        std::printf("%s | small_c10=%d mid=%d p10_floats=%zu inp0sf_floats=%zu c10part_floats=%zu merge_stride=%d\n", pfnl::plan_text(pl).c_str(),
                    pl.small_c10 ? 1 : 0, pl.mid || pl.bmid ? 1 : 0, pl.p10_floats, pl.inp0sf_floats, pl.c10part_floats, pl.merge_stride);
    }
    return 0;
}
"""


def build(tmp_dir, extra_flags=()):
    """Compiles the driver into tmp_dir (skips the calling test without hipcc); returns run(queries) -> [(plan text, extras text)]."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc")
    src, exe = tmp_dir / "plan_driver.cpp", tmp_dir / "plan_driver"
    src.write_text(DRIVER)
    r = subprocess.run([hipcc, "-O1", "-std=c++17", *extra_flags, "-I", os.path.join(ROOT, "pfnl_amd", "csrc"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr

    def run(queries):
        p = subprocess.run([str(exe)], input="\n".join(queries) + "\n", capture_output=True, text=True)
        assert p.returncode == 0, (p.returncode, p.stderr)
        out = p.stdout.split("\n")
        assert len(out) == len(queries) + 1
        return [tuple(o.split(" | ")) for o in out[:-1]]

    return run


def fields(text):
    """"name k=v ..." (or only "k=v ...") -> dict, integers as int, the name under "structure"."""
    d = {}
    for t in text.split():
        k, eq, v = t.partition("=")
        if not eq:
            d["structure"] = t
        else:
            d[k] = int(v) if v.lstrip("-").isdigit() else v
    return d


def nl_fits_of(plan_text):
    """The nl_fits input that belongs to a reported plan: where the non-local block runs on the f16 pipe the plan's nl_pack_fused IS that
    answer; elsewhere the plan does not read it."""
    d = fields(plan_text)
    return d["nl_pack_fused"] if d["nl"] in ("split16", "f16") else 1
