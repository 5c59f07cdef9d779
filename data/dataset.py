"""`from data import dataset` as in the reference's test_cvo.py:5."""
from accflow_amd.data.dataset import (CVO, CVO_sampler_lmdb, High_Speed_Sintel, SyntheticCVO,  # noqa: F401
                                      fetch_sintel_dataloader, fetch_valid_dataloader, totensor)
