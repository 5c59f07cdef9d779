from accflow_amd.networks.AccFlow_ import (AccFlow, AccFlowStream, AccPlus, Blending, FlowDecoder, FlowEncoder,  # noqa: F401
                                            downflow8, getOcc)
