"""Builds of mdil_ss_amd/ext/density_head.hip that differ from what ships in ONE constant each (the -D switches at
the top of that file), timed one after the other in one process: ``profiles/density_variants.txt``.

    python tools/bench_density_variants.py --build-dir DIR --build-only      # compile the variants (no GPU needed)
    python tools/bench_density_variants.py --build-dir DIR [--out FILE]      # time them on an MI355X

``density_head`` on 6 x 256 x 512 x 16 features at 20 classes and ``density_rows`` on 6 x 64 x 128 rows of 128 channels,
each as [with both histograms, with the maha histogram, without a histogram], on a randomly initialised network's
features ("net"), all-zero features ("zero") and clustered features with 5 % far rows ("clustered"); median of
``--rounds`` rounds of ``--iters`` calls, microseconds.  Every build must give the shipped build's histogram bytes."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VARIANTS = {
    "ships": [],
    "rows_model_from_global": ["-DMDIL_DENSITY_ROWS_MODEL_IN_LDS=0"],
    "rows_blocks_512": ["-DMDIL_DENSITY_ROWS_BLOCKS=512"],
    "rows_blocks_1024": ["-DMDIL_DENSITY_ROWS_BLOCKS=1024"],
    "head_waves_2": ["-DMDIL_DENSITY_HEAD_WAVES=2"],
    "head_blocks_512": ["-DMDIL_DENSITY_HEAD_BLOCKS=512"],
    "merge_rounds_2": ["-DMDIL_DENSITY_MERGE_ROUNDS=2"],
    "no_merge": ["-DMDIL_DENSITY_MERGE_ROUNDS=1", "-DMDIL_DENSITY_MIN_MERGED=65"],
}


def build(build_dir):
    ext = os.path.join(ROOT, "mdil_ss_amd", "ext")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    os.makedirs(build_dir, exist_ok=True)
    for name, flags in VARIANTS.items():
        obj, lib = os.path.join(build_dir, name + ".o"), os.path.join(build_dir, f"libmdil_density_{name}.so")
        subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", *flags, "-c",
                        os.path.join(ext, "density_head.hip"), "-o", obj], check=True)
        subprocess.run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC",
                        "-Wl,--version-script=" + os.path.join(ext, "density_exports.map"), obj, "-o", lib], check=True)
        os.remove(obj)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build-dir", required=True)
    ap.add_argument("--build-only", action="store_true")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", help="also write the lines here")
    args = ap.parse_args()
    if args.build_only:
        build(args.build_dir)
        return
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_density_variants needs an MI355X")
    from mdil_ss_amd import _addon_lib, _density_lib, latent
    from mdil_ss_amd import density as D
    from mdil_ss_amd.models.erfnet_RA_parallel import Net
    from tools import bench_density as BD
    from tools._bench_common import timed
    if not all(os.path.exists(os.path.join(args.build_dir, f"libmdil_density_{n}.so")) for n in VARIANTS):
        build(args.build_dir)
    dev, nc = torch.device("cuda", 0), 20
    torch.manual_seed(0)
    net = Net([nc], 1, 0).to(dev).eval()
    images = torch.rand(6, 3, 512, 1024, device=dev)
    with torch.no_grad():
        feat = net.features(images, 0).contiguous()
        w, b = (t.detach().contiguous() for t in net.head_params(0))
    enc = latent.latents(net, images, 0, "encoder").view(-1, 128)
    inputs = {}
    for form, rows in (("head", feat.view(-1, 16)), ("rows", enc)):
        n, C = rows.shape
        labels = torch.randint(0, nc - 1, (n,), generator=torch.Generator().manual_seed(1)).to(torch.uint8).to(dev)
        cx, cl = BD.clustered(C, nc - 1, n, 2, dev)
        nm, cm = D.DeviceModel(BD.fit_to(rows, labels, nc - 1), dev), D.DeviceModel(BD.fit_to(cx, cl, nc - 1), dev)
        shape = feat.shape if form == "head" else rows.shape
        inputs[form] = {"net": (rows.view(shape), nm), "zero": (torch.zeros(shape, device=dev), nm),
                        "clustered": (cx.view(shape), cm)}
    hist = torch.zeros(2, 2, 65536, dtype=torch.int64, device=dev)
    nonf, agree = torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(2, dtype=torch.int64, device=dev)

    def calls(form, x, dm):
        if form == "head":
            return (lambda: D.density_head(x, w, b, dm, map_kind="maha", hist=hist, nonfinite=nonf, agree=agree),
                    lambda: D.density_head(x, w, b, dm, map_kind="maha", kinds=["maha"], hist=hist),
                    lambda: D.density_head(x, w, b, dm, map_kind="maha"))
        return (lambda: D.density_rows(x, dm, map_kind="maha", hist=hist, nonfinite=nonf),
                lambda: D.density_rows(x, dm, map_kind="maha", kinds=["maha"], hist=hist),
                lambda: D.density_rows(x, dm, map_kind="maha"))

    lines, ref = [], {}
    for name in list(VARIANTS) + ["ships"]:                         # what ships is measured first and last
        path = os.path.join(args.build_dir, f"libmdil_density_{name}.so")
        _density_lib.load, _density_lib.check = _addon_lib.bind(path, _density_lib._SIGNATURES, "mdil_density", "density")
        out = {}
        for form in ("head", "rows"):
            out[form] = {}
            for iname, (x, dm) in inputs[form].items():
                hist.zero_()
                calls(form, x, dm)[0]()
                torch.cuda.synchronize()
                assert torch.equal(ref.setdefault((form, iname), hist.clone()), hist), (name, form, iname)
                out[form][iname] = []
                for fn in calls(form, x, dm):
                    timed(fn, 3)
                    out[form][iname].append(round(statistics.median([timed(fn, args.iters) for _ in range(args.rounds)]), 1))
        lines.append(f"{name:24s} {' '.join(VARIANTS[name]) or '(no switch)'}\n    [2 hists, maha hist, no hist] us: "
                     + json.dumps(out))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
