"""python -m graphchainer_amd: the command line of graphchainer_amd/cli.py."""
import sys

from .cli import main

sys.exit(main())
