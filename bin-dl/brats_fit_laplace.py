#!/usr/bin/env python3
"""brats Laplace fit (EXTENSION, not in the reference): fits the last-layer Laplace approximation on the volumes a test
config's test_data names and writes laplace.npz and laplace.json into the run directory (rcu_amd.scripts.fit_laplace)."""
import argparse
import logging
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

if __name__ == '__main__':
    try:
        parser = argparse.ArgumentParser(description='brats Laplace fit (EXTENSION: last-layer Laplace uncertainty)')
        parser.add_argument('-config_file', type=str, help='the test configuration (test_data: the volumes to fit on)')
        args = parser.parse_args()
        from rcu_amd import scripts
        scripts.fit_laplace('brats', args.config_file)
    finally:
        logging.exception('')  # log the exception
