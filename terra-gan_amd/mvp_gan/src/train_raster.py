"""Fine-tune the inpainting GAN on one DSM raster in metres.

Train and validation windows come from RasterWindowLoader (utils/raster_dataset.py) on the geographic split of the raster
(train and val blocks never share a pixel); holes are synthetic.  The checkpoint written to --out has the reference's keys
(train.py's dictionary) and loads unchanged into `inpaint_raster --checkpoint`.

CLI: python -m mvp_gan.src.train_raster --dem in.asc [--mask keep.png|keep.asc] [--nodata v] [--init ck.pth] --out ft.pth
         [--window 256 --batch 16 --steps 500 --epochs 4 --seed 0 --norm known|window] [--remove-objects [spec flags]]
         [--model-cellsize 1.0 [--min-coverage 0.5]] [--evaluate [--eval-json report.json]]

--evaluate scores the written checkpoint on held-out holes of the test split (mvp_gan/src/evaluate_raster.py) with the same
block, window (as the hole tile), seed, nodata, mask and objects, prints one line and writes the report to --eval-json.

--remove-objects finds the above-ground objects in the DSM (mvp_gan/src/object_mask.py, cellsize from the header) and never
samples a window that touches one, so the generator learns bare earth.

--model-cellsize resamples the raster, the mask and the object keep-mask once to that cell size (mvp_gan/src/resample.py,
DESIGN.md section 8m; the raster's own comes from the header): the checkpoint is fine-tuned at the cell size it will be used
at, and --window and --block are in resampled pixels.  --evaluate then scores it with the same model cell size and coverage on
the native grid, where the holes are cut: block and tile are the same ground squares counted in native pixels (block x
scale, window x scale; evaluate_raster.native_cells), so a test cell still shares no ground with a train or val block.  That
needs both products to be whole numbers and the tile within evaluate_raster's range; a run that cannot be scored this way is
refused before it trains.
"""
import argparse
import logging

import torch

from .asc import read_inputs
from .models.discriminator import Discriminator
from .models.generator import PConvUNet
from .object_mask import add_spec_args, spec_from_args
from .train import _default_config, train
from .utils.raster_dataset import RasterWindowLoader


def _load_init(path, generator, discriminator, optimizer_G, optimizer_D, device):
    """Generator weights (a train() checkpoint or a bare state dict), plus the discriminator and optimiser states when the
    checkpoint has them.  -> the names of what was loaded."""
    ck = torch.load(path, map_location=device, weights_only=False)
    if not (isinstance(ck, dict) and "generator_state_dict" in ck):
        generator.load_state_dict(ck)
        return ["generator"]
    generator.load_state_dict(ck["generator_state_dict"])
    loaded = ["generator"]
    for key, obj in (("discriminator_state_dict", discriminator), ("optimizer_G_state_dict", optimizer_G),
                     ("optimizer_D_state_dict", optimizer_D)):
        if key in ck:
            obj.load_state_dict(ck[key])
            loaded.append(key.replace("_state_dict", ""))
    return loaded


def build_parser():
    ap = argparse.ArgumentParser(description="Fine-tune a TERRA-GAN generator on windows of one ESRI ASCII grid DSM.")
    ap.add_argument("--dem", required=True, help="input .asc raster in metres (NODATA_value cells are never sampled)")
    ap.add_argument("--mask", help="optional mask (.png or .asc) of the raster's size: nonzero = usable, 0 = never sampled")
    ap.add_argument("--nodata", type=float, help="nodata value (default: the .asc header's NODATA_value)")
    ap.add_argument("--init", help="checkpoint to start from: generator, plus discriminator / optimiser states if present")
    ap.add_argument("--out", required=True, help="output checkpoint (.pth), reference format")
    ap.add_argument("--window", type=int, default=256)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--steps", type=int, default=500, help="train steps per epoch")
    ap.add_argument("--val-steps", type=int, help="validation batches per epoch (default: max(1, steps // 10))")
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--block", type=int, help="side of the train / val / test blocks (default: 4 x window)")
    ap.add_argument("--lr", type=float, default=2e-4)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--norm", choices=("known", "window"), default="known")
    ap.add_argument("--remove-objects", action="store_true",
                    help="never sample windows that touch an above-ground object found in the DSM")
    ap.add_argument("--model-cellsize", type=float,
                    help="train on the raster resampled to this cell size (the raster's own comes from the header)")
    ap.add_argument("--min-coverage", type=float, default=0.5,
                    help="with a coarser --model-cellsize: the known share of its footprint a resampled cell needs, in (0, 1]")
    ap.add_argument("--evaluate", action="store_true", help="score the written checkpoint on held-out holes of the test split")
    ap.add_argument("--eval-json", help="with --evaluate: write the report here")
    add_spec_args(ap)
    return ap


def main(argv=None):
    ap = build_parser()
    a = ap.parse_args(argv)
    if a.eval_json and not a.evaluate:
        ap.error("--eval-json needs --evaluate")
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    if not torch.cuda.is_available():
        raise RuntimeError("train_raster: no HIP device visible; this build has no CPU path")
    device = torch.device("cuda", torch.cuda.current_device())

    dem, _, mask, nodata, cellsize = read_inputs(a)
    common = dict(nodata=nodata, window=a.window, batch_size=a.batch, block=a.block, norm=a.norm, seed=a.seed, device=device)
    if a.remove_objects:
        common.update(objects=spec_from_args(a), cellsize=cellsize)
    if a.model_cellsize is not None:
        common.update(model_cellsize=a.model_cellsize, min_coverage=a.min_coverage,
                      cellsize=cellsize)
    tr = RasterWindowLoader(dem, mask, split="train", steps_per_epoch=a.steps, **common)
    va = RasterWindowLoader(dem, mask, split="val", steps_per_epoch=a.val_steps or max(1, a.steps // 10), augment=False,
                            **common)
    if a.evaluate:                               # the plan of the scoring, checked before the training it would follow
        from .evaluate_raster import HoleSpec, check_plan, native_cells
        from .inpaint_raster import check_resample_options
        scale = check_resample_options(common.get("cellsize"), a.model_cellsize, a.min_coverage, who="train_raster")
        eval_block, eval_tile = native_cells(tr.block, a.window, scale, who="train_raster --evaluate")
        check_plan(*dem.shape, "test", eval_block, eval_tile, HoleSpec(), who="train_raster --evaluate")

    torch.manual_seed(a.seed)
    G, D = PConvUNet().to(device), Discriminator().to(device)
    oG = torch.optim.Adam(G.parameters(), lr=a.lr)
    oD = torch.optim.Adam(D.parameters(), lr=a.lr)
    loaded = _load_init(a.init, G, D, oG, oD, device) if a.init else []
    cfg = _default_config()
    cfg["training"].update(batch_size=a.batch, learning_rate=a.lr, epochs=a.epochs, seed=a.seed)
    res = train(tr, None, generator=G, discriminator=D, optimizer_G=oG, optimizer_D=oD, checkpoint_path=a.out, config=cfg,
                val_img_dir=va)
    print(f"{a.out}: {a.epochs} epochs x {a.steps} steps of {a.batch} windows {a.window}^2 "
          f"(admissible train {tr.info['admissible_fraction']:.3f}, val {va.info['admissible_fraction']:.3f}), "
          f"init {'+'.join(loaded) or 'random'}, best val g_loss {res['best_val_loss']:.5f}")
    if a.evaluate:
        import json

        from .evaluate_raster import evaluate_raster, summary
        rep, _ = evaluate_raster(a.out, dem, mask, nodata=nodata, cellsize=cellsize, split="test",
                                 block=eval_block, tile=eval_tile, seed=a.seed, objects=common.get("objects"),
                                 model_cellsize=a.model_cellsize, min_coverage=a.min_coverage)
        if a.eval_json:
            with open(a.eval_json, "w") as f:
                json.dump(rep, f, indent=1)
        print(f"test split: {summary(rep)}")
        res["evaluation"] = rep
    return res


if __name__ == "__main__":
    main()
