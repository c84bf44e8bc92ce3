#!/usr/bin/env python3
"""Entry point of the 3-D nets (NVNet3D / UNet3D), the counterpart of `main_missing.py`: reads `config3d.yaml` (or the file named first on
the command line, then key=value overrides), trains with a validation pass per epoch, scores the test set, or writes whole-volume label maps (phase=predict) on the MI355X hot path.

    python main_3d.py                            # config3d.yaml in the working directory, else the built-in defaults
    python main_3d.py cfg3d.yaml epochs=2 batch_size=2 ckpt_path=/tmp/ckpt3d
    python main_3d.py cfg3d.yaml patch_size=[128,128,128] patch_fg=0.33  # train on random 128^3 patches of the whole scan, a third of them on the tumour
    python main_3d.py cfg3d.yaml phase=test
    python main_3d.py cfg3d.yaml phase=predict   # <ckpt_path>/result_test/<subj_id>_seg.npy + predict.csv
    python main_3d.py cfg3d.yaml phase=predict predict_regions=true     # + predict_regions.csv: Dice, sensitivity, specificity, HD95 of WT / TC / ET
    python main_3d.py cfg3d.yaml phase=score     # the same csv for label volumes already under result_test/ (no model is built or loaded)
    python main_3d.py cfg3d.yaml phase=predict predict_post=true post_min_voxels=50     # + post/<subj_id>_seg.npy cleaned by connected components, post/postprocess.csv
    python main_3d.py cfg3d.yaml phase=postprocess post_keep=largest    # the same post/ files from label volumes already under result_test/ (no model)
    python main_3d.py cfg3d.yaml phase=score score_subdir=post          # region scores of the cleaned volumes
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mrdis  # noqa: E402

if __name__ == '__main__':
    mrdis.train3d.main()
