#!/usr/bin/env python3
"""Record what the reference's own acrobot, cart-pole, pendulum and compass-walker code answers on the case sets of
tests/ref_env_cases.py, and its tile coding on those of tests/ref_tile_cases.py.

Needs oracle/_ref/ref_envs, oracle/_ref/ref_envs_fused and oracle/_ref/ref_tiles (`make -C oracle` on a machine with a checkout of
the reference).
Writes
  tests/golden/ref_envs_{acrobot,walker,cart_pole,pendulum}.npz   inputs and the binary's outputs: data only
  tests/golden/ref_tiles.npz   tile coding specs, inputs and the indices oracle/_ref/ref_tiles answered: data only
  tests/golden/ref_envs_bounds.json   per environment and output group the largest absolute deviation of the PORTABLE-mode
      oracle (what the kernels reproduce bit for bit) from the binary on those rows -- measured against the reference, never
      against a kernel --, the rows excluded for a different discrete outcome, the rows on which a binary built at plain -O2
      (g++ fuses sin/cos into sincos) differs from the call-by-call one, and the compiler and C library that built both.
tests/test_oracle_ref_envs.py and tests/test_oracle_ref_tiles.py hold the files against a fresh run; tests/test_gpu_ref_envs.py and
tests/test_gpu_ref_tiles.py read them on the GPU.
Run:  python tools/record_ref_envs.py
"""
import json
import os
import platform
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import oracle_binding as ob  # noqa: E402
from tests import ref_env_cases as rc  # noqa: E402
from tests import ref_tile_cases as tc  # noqa: E402


ENVS = ("acrobot", "walker", "cart_pole", "pendulum")


def differing_rows(a, b, keys):
    bad = np.zeros(len(a[keys[0]]), bool)
    for k in keys:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        if x.dtype == np.float64:
            x, y = x.view(np.uint64), y.view(np.uint64)
        bad |= (x != y).reshape(len(bad), -1).any(axis=1)
    return bad


def record(env):
    cases = rc.CASES[env]()
    ref = rc.reference_answers(env, cases)
    portable = rc.oracle_answers(env, cases, ob.MATH_PORTABLE)
    excluded = rc.discrete_mismatch(env, ref, portable)
    starts = rc.context_starts(env)
    sref = rc.reference_starts(env, starts)
    sportable = rc.oracle_starts(env, starts, ob.MATH_PORTABLE)
    sexcluded = sref["position_after"] != sportable["position_after"]
    fused = rc.reference_answers(env, cases, rc.REF_BIN_FUSED)
    sfused = rc.reference_starts(env, starts, rc.REF_BIN_FUSED)
    out = dict(cases)                                                     # state, action, tag (and the cart-pole's variant)
    out.update(next=ref["next"], obs=ref["obs"], reward=ref["reward"], term=ref["term"], excluded=excluded)
    out.update({"start_" + k: v for k, v in starts.items()})              # position, test (and the randomization where there is one)
    out.update(start_x=sref["x"], start_obs=sref["obs"], start_position_after=sref["position_after"], start_excluded=sexcluded)
    np.savez_compressed(rc.FIXTURE[env], **out)
    keys = rc.ANSWER_KEYS[env]
    return {"rows": int(len(excluded)), "excluded_rows": int(excluded.sum()),
            "bounds": rc.deviations(env, ref, portable, excluded),
            "starts": int(len(sexcluded)), "excluded_starts": int(sexcluded.sum()),
            "start_bounds": rc.start_deviations(env, sref, sportable, sexcluded),
            "rows_differing_at_plain_O2": int(differing_rows(ref, fused, keys).sum()),
            "starts_differing_at_plain_O2": int(differing_rows(sref, sfused, ("x", "obs", "position_after")).sum())}


def record_tiles():
    """tests/golden/ref_tiles.npz: per spec k its shape, its inputs x{k}, their tags tag{k} and what oracle/_ref/ref_tiles answered, idx{k};
    the names of the specs configure() refuses, those a fixed-size spec can say with their shapes.  Data only."""
    specs, refused = tc.specs(), tc.refused_specs()
    for s in refused:
        assert tc.reference_refuses(s), s["name"]

    def shapes(which):
        res, wrap = np.zeros((len(which), tc.MAX_DIMS)), np.zeros((len(which), tc.MAX_DIMS))
        for k, s in enumerate(which):
            res[k, :len(s["res"])] = s["res"]; wrap[k, :len(s["wrap"])] = s["wrap"]
        return dict(names=np.array([s["name"] for s in which]), tilings=np.array([s["tilings"] for s in which], np.int32),
                    memory=np.array([s["memory"] for s in which], np.int32), dims=np.array([len(s["res"]) for s in which], np.int32),
                    wrap_len=np.array([len(s["wrap"]) for s in which], np.int32), res=res, wrap=wrap)
    out = shapes(specs)
    out.update({"refused_" + k: v for k, v in shapes(refused).items()})
    rows = 0
    for k, s in enumerate(specs):
        cases = tc.inputs(s, seed=7000 + k)
        out[f"x{k}"], out[f"tag{k}"], out[f"idx{k}"] = cases["x"], cases["tag"], tc.reference_indices(s, cases["x"])
        rows += len(cases["tag"])
    np.savez_compressed(tc.FIXTURE, **out)
    return {"specs": len(specs), "refused_specs": len(refused), "rows": rows}


def main():
    out = {env: record(env) for env in ENVS}
    pool = rc.walker_pool()                                              # the 12 k steps the walker's rows are chosen from
    call_by_call, fused = rc.reference_answers("walker", pool), rc.reference_answers("walker", pool, rc.REF_BIN_FUSED)
    differ = differing_rows(call_by_call, fused, rc.ANSWER_KEYS["walker"])
    largest = max(float(np.max(np.abs(call_by_call[k][differ] - fused[k][differ]))) for k in ("next", "obs", "reward")) if differ.any() else 0.0
    out["walker"]["pool_rows"] = int(len(differ))
    out["walker"]["pool_rows_differing_at_plain_O2"] = int(differ.sum())
    out["walker"]["pool_largest_difference_at_plain_O2"] = largest
    out["walker"]["pool_discrete_differences_at_plain_O2"] = int(rc.discrete_mismatch("walker", call_by_call, fused).sum())
    out["tiles"] = record_tiles()
    out["toolchain"] = {"compiler": subprocess.run(["g++", "--version"], capture_output=True, text=True, check=True).stdout.splitlines()[0],
                        "libc": " ".join(platform.libc_ver()),
                        "flags": "-O2 -std=c++11 -ffp-contract=off -fno-builtin (plain -O2: without -fno-builtin)"}
    with open(rc.BOUNDS, "w") as f:
        json.dump(out, f, indent=2, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, indent=2, sort_keys=True))
    print(tc.FIXTURE, os.path.getsize(tc.FIXTURE), "bytes")
    for env in ENVS:
        print(rc.FIXTURE[env], os.path.getsize(rc.FIXTURE[env]), "bytes")


if __name__ == "__main__":
    main()
