#!/usr/bin/env python3
"""isic temperature fit (EXTENSION, not in the reference): fits T on the validation volumes a test config's test_data names and writes
temperature.json into the run directory (rcu_amd.scripts.fit_temperature)."""
import argparse
import logging
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

if __name__ == '__main__':
    try:
        parser = argparse.ArgumentParser(description='isic temperature fit (EXTENSION: temperature scaling)')
        parser.add_argument('-config_file', type=str, help='the test configuration (test_data: the validation volumes)')
        args = parser.parse_args()
        from rcu_amd import scripts
        scripts.fit_temperature('isic', args.config_file)
    finally:
        logging.exception('')  # log the exception
