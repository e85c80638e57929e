#!/usr/bin/env python3
"""brats density fit (EXTENSION, not in the reference): fits the class Gaussians of the feature-space density on the validation volumes a test
config's test_data names and writes density.npz and density.json into the run directory (rcu_amd.scripts.fit_density)."""
import argparse
import logging
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

if __name__ == '__main__':
    try:
        parser = argparse.ArgumentParser(description='brats density fit (EXTENSION: feature-space density uncertainty)')
        parser.add_argument('-config_file', type=str, help='the test configuration (test_data: the validation volumes)')
        args = parser.parse_args()
        from rcu_amd import scripts
        scripts.fit_density('brats', args.config_file)
    finally:
        logging.exception('')  # log the exception
