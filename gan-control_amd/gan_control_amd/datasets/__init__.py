from .dataframe_dataset import DataFrameDataSet, DeviceFrame, get_dataframe_data_loader

__all__ = ['DataFrameDataSet', 'DeviceFrame', 'get_dataframe_data_loader']
