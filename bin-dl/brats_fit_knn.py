#!/usr/bin/env python3
"""brats k-NN bank fit (EXTENSION, not in the reference): samples the bank of the nearest-neighbour feature uncertainty on the validation volumes a test
config's test_data names and writes knn.npz and knn.json into the run directory (rcu_amd.scripts.fit_knn)."""
import argparse
import logging
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

if __name__ == '__main__':
    try:
        parser = argparse.ArgumentParser(description='brats k-NN bank fit (EXTENSION: nearest-neighbour feature uncertainty)')
        parser.add_argument('-config_file', type=str, help='the test configuration (test_data: the validation volumes)')
        args = parser.parse_args()
        from rcu_amd import scripts
        scripts.fit_knn('brats', args.config_file)
    finally:
        logging.exception('')  # log the exception
