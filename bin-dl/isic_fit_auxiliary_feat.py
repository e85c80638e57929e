#!/usr/bin/env python3
"""isic auxiliary fit (EXTENSION; the reference's isic_train_auxiliary_feat.py as a post-hoc fit): fits the auxiliary PostNet on the features of the
frozen segmentation model of a test config, on the volumes its test_data names, and writes a PostNet model directory, auxiliary_fit.json and
auxiliary_fit.csv into the run directory (rcu_amd.scripts.fit_auxiliary_feat)."""
import argparse
import logging
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

if __name__ == '__main__':
    try:
        parser = argparse.ArgumentParser(description='isic auxiliary fit (EXTENSION: the auxiliary feature network from a U-Net checkpoint)')
        parser.add_argument('-config_file', type=str, help='the test configuration (model_dir: the segmentation model; test_data: the volumes to fit on)')
        args = parser.parse_args()
        from rcu_amd import scripts
        scripts.fit_auxiliary_feat('isic', args.config_file)
    finally:
        logging.exception('')  # log the exception
