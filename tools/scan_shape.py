"""Scan shape and resources of the specialised render kernel of a bench workload (option "scan_jit", rpt_scan_jit_info): one small
render with the option forced, then the query -- shape string, state and reason, where the code object came from, compile time,
VGPRs and scratch of the code object beside the AOT kernel's VGPRs.
Usage (GPU box, from the repo root): python tools/scan_shape.py [workload ...]        (default: C3 C2)"""
import json
import sys

sys.path.insert(0, ".")
from rpt_amd import Renderer, scenes  # noqa: E402


def main():
    for name in sys.argv[1:] or ["C3", "C2"]:
        scene, cam, cfg = scenes.CONFIGS[name]()
        scene.set_option("scan_jit", 2)
        r = Renderer(scene, cam).width(64).height(64).max_bounces(cfg["max_bounces"]).seed(1)
        r.sample_array(2)
        print(name, json.dumps(r.scan_jit_info()), flush=True)


if __name__ == "__main__":
    main()
